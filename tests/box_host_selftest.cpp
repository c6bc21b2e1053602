// Box shapes (extension, include/flux_abi.h FLUX_SHAPE_BOX) in the C++ host layer and the host scene build, CPU only
// (tests/test_box_scene.py builds and runs it, once more under AddressSanitizer and UBSan): the YAML loader and its corner checks, the
// optional `invert`, the conversion to flux_shape, a CBOR round trip through the node protocol's SetJob message, and the host scene
// build's records -- six hit records per box with the right normals and ids, and unchanged bytes for a scene without boxes.
//   usage: box_host_selftest <scenes dir>
// Prints "shape <i> <fields>" for every flux_shape of scenes/box_room.yml (compared with the Python loader by the test), one
// "ok <name>" per passed check and "all ok" at the end; exits 1 on the first failure.
#include <cmath>
#include <cstring>
#include <string>

#include "../flux_amd/csrc/flux_plan.h"
#include "../flux_amd/csrc/scene_build.h"
#include "host_selftest.hpp"

int main(int argc, char **argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <scenes dir>\n", argv[0]);
        return 2;
    }
    const std::string path = std::string(argv[1]) + "/box_room.yml";
    const SceneData sd = scene_from_yaml_file(path);
    CHECK(sd.shapes.size() == 5);
    const BoxData *room = std::get_if<BoxData>(&sd.shapes[0]);
    const BoxData *table = std::get_if<BoxData>(&sd.shapes[2]);
    CHECK(room != nullptr && table != nullptr && std::holds_alternative<DiskData>(sd.shapes[1]));
    CHECK(room->invert && room->corner0.x == -8.0 && room->corner1.z == 8.0);
    CHECK(!table->invert && table->corner1.y == 2.0);  // no `invert` in the file: false
    const AbiScene abi(sd);
    {
        CHECK(abi.desc.num_shapes == 5 && abi.shapes[0].kind == FLUX_SHAPE_BOX && FLUX_SHAPE_BOX == 3 && abi.shapes[0].invert == 1);
        CHECK(abi.shapes[2].kind == FLUX_SHAPE_BOX && abi.shapes[2].invert == 0 && abi.shapes[2].p[0] == -5.0 && abi.shapes[2].n[2] == 4.5);
        print_flux_shapes(abi);
        std::printf("ok abi scene\n");
    }
    {   // the loader's corner checks: the field's path in every message
        const std::string good = read_file(path);
        const std::string c0 = "      corner0: [-5.0, 0.0, 1.0]\n", c1 = "      corner1: [-1.5, 2.0, 4.5]\n";
        CHECK(good.find(c0) != std::string::npos && good.find(c1) != std::string::npos);
        CHECK(throws(replaced(good, c0, ""), "shapes[2].Box: missing field `corner0`"));
        CHECK(throws(replaced(good, c1, ""), "shapes[2].Box: missing field `corner1`"));
        CHECK(throws(replaced(good, c1, "      corner1: [1, 2]\n"), "shapes[2].Box.corner1"));
        CHECK(throws(replaced(good, c1, "      corner1: big\n"), "shapes[2].Box.corner1"));
        CHECK(throws(replaced(good, c0, "      corner0: [nan, 0.0, 1.0]\n"), "shapes[2].Box.corner0"));
        CHECK(throws(replaced(good, c0, "      corner0: [-5.0, -inf, 1.0]\n"), "shapes[2].Box.corner0"));
        CHECK(throws(replaced(good, c1, "      corner1: [-1.5, 2.0, inf]\n"), "shapes[2].Box.corner1"));
        CHECK(throws(replaced(good, c1, "      corner1: [-1.5, nan, 4.5]\n"), "shapes[2].Box.corner1"));
        CHECK(throws(replaced(good, c1, "      corner1: [-5.0, 2.0, 4.5]\n"), "shapes[2].Box.corner1: expected finite numbers above corner0 (axis x)"));
        CHECK(throws(replaced(good, c1, "      corner1: [-1.5, -1.0, 4.5]\n"), "shapes[2].Box.corner1: expected finite numbers above corner0 (axis y)"));
        CHECK(throws(replaced(good, c1, "      corner1: [-1.5, 2.0, 1.0]\n"), "shapes[2].Box.corner1: expected finite numbers above corner0 (axis z)"));
        CHECK(throws(replaced(good, c1, c1 + "      invert: 3\n"), "shapes[2].Box.invert"));
        const SceneData inv = scene_from_yaml_text(replaced(good, c1, c1 + "      invert: true\n"));
        CHECK(std::get<BoxData>(inv.shapes[2]).invert);
        std::string unknown = good;
        unknown.replace(unknown.find("- Disk:"), 7, "- Quad:");
        CHECK(throws(unknown, "unknown variant `Quad`, expected one of `Sphere`, `Plane`, `Disk`, `Box`"));
        std::printf("ok yaml corners\n");
    }
    {   // CBOR: SetJob with the box scene, decoded back field for field and re-encoded to the same bytes
        std::string raw;
        NetworkWorkerRequest back;
        if (set_job_round_trip(sd, raw, back)) return 1;
        CHECK(raw.find("Box") != std::string::npos && raw.find("corner1") != std::string::npos);
        const BoxData *b = std::get_if<BoxData>(&back.job.scene_data.shapes[0]);
        CHECK(b != nullptr && same_vec(b->corner0, room->corner0) && same_vec(b->corner1, room->corner1) && b->invert);
        const BoxData *g = std::get_if<BoxData>(&back.job.scene_data.shapes[3]);
        CHECK(g != nullptr && !g->invert && std::holds_alternative<GlossyReflectiveData>(g->material));
        NetworkWorkerRequest req = back;  // the same scene: it re-encoded to the same bytes
        req.job.scene_data.shapes.push_back(BoxData{Vec3{0.1, -2.5, -1e300}, Vec3{1.0 / 3.0, 0, 1e300}, EmissiveData{Color{1, 2, 3}, 0.5}, true});
        cbor::Encoder e3;
        encode_request(e3, req);
        cbor::StringReader r3(e3.out);
        cbor::Decoder d3(r3);
        NetworkWorkerRequest back3;
        CHECK(decode_request(d3, back3));
        const BoxData *t = std::get_if<BoxData>(&back3.job.scene_data.shapes.back());
        CHECK(t && t->invert && t->corner1.x == 1.0 / 3.0 && t->corner0.z == -1e300 && std::holds_alternative<EmissiveData>(t->material));
        std::printf("ok cbor round trip\n");
    }
    {   // the host scene build: records in scan order (1 sphere, 0 planes, 1 disk, then six per box in YAML order)
        flux::HostScene h;
        std::string err;
        CHECK(flux::build_host_scene(abi.desc, h, err) == FLUX_OK);
        const flux::RenderParams &p = h.rp;
        CHECK(p.n_sph == 1 && p.n_pln == 0 && p.n_dsk == 1 && p.n_box == 3 && flux::hit_records(p) == 20 && p.n_shapes == 5);
        CHECK(p.glossy_long == 0 && p.unit_dirs == 1 && p.self_skip == 1 && p.has_diel == 0);
        CHECK(h.fs.box == h.fs.dsk + 2 * sizeof(flux::DevScanDisk) && h.fs.bytes == h.fs.box + 3 * sizeof(flux::DevScanBox));
        CHECK(h.fs.s32 >= h.fs.rec + 21 * sizeof(flux::DevHitRec) && h.fscene.size() == h.fs.bytes);
        const flux::DevHitRec *rec = reinterpret_cast<const flux::DevHitRec *>(h.fscene.data() + h.fs.rec);
        const flux::DevScanBox *box = reinterpret_cast<const flux::DevScanBox *>(h.fscene.data() + h.fs.box);
        CHECK(rec[0].orig_id == 4 && rec[0].shape_kind == flux::kShapeSphere && rec[1].orig_id == 1 && rec[1].shape_kind == flux::kShapeDisk);
        const int ids[3] = {0, 2, 3};
        const int mats[3] = {flux::kMatMatte, flux::kMatMatte, flux::kMatGlossy};
        for (int j = 0; j < 3; j++) {
            const flux_shape &s = abi.shapes[ids[j]];
            CHECK(box[j].id == ids[j] && box[j].inv == (s.invert ? -1.0 : 1.0));
            CHECK(box[j].c0x == s.p[0] && box[j].c0y == s.p[1] && box[j].c0z == s.p[2]);
            CHECK(box[j].c1x == s.n[0] && box[j].c1y == s.n[1] && box[j].c1z == s.n[2]);
            for (int face = 0; face < 6; face++) {
                const flux::DevHitRec &r = rec[2 + 6 * j + face];
                const double n[3] = {r.cx, r.cy, r.cz};
                CHECK(r.orig_id == ids[j] && r.mat_kind == mats[j] && r.shape_kind != flux::kShapeSphere && r.unit_normal == 1);
                for (int a = 0; a < 3; a++)
                    CHECK(n[a] == (a == face / 2 ? ((face & 1) ? 1.0 : -1.0) * box[j].inv : 0.0) && !std::signbit(a == face / 2 ? 0.0 : n[a]));
                CHECK(r.fr == rec[2 + 6 * j].fr && r.fg == rec[2 + 6 * j].fg && r.fb == rec[2 + 6 * j].fb && r.inv_e1 == rec[2 + 6 * j].inv_e1);
                CHECK(r.ax == rec[2 + 6 * j].ax && r.az == rec[2 + 6 * j].az && r.inv_rad == 0.0);
            }
        }
        // the glossy angle table: one exponent slot each for the sphere's and the glossy box's exponents; every face of that box shares its slot
        CHECK(p.n_gloss_exp == 2 && p.gx_stride == 32 && h.gx_off.size() == 21);
        for (int face = 0; face < 6; face++) CHECK(h.gx_off[2 + 12 + face] == h.gx_off[2 + 12]);
        CHECK(h.gx_off[0] != h.gx_off[14]);
        // the launch plan: the split kernel's general instantiation.  At 256 spp a block is one wave and the LDS a wave may have at
        // five waves a SIMD holds no queue of 64 + FLUX_HITQ_MIN_TAKE slots beside 1 952 B of records (nor beside demo2's 1 632 B);
        // from two waves a pixel on the block's share holds the hit queue
        static const flux::DevScanSphere32 placeholder{};
        for (const uint32_t root : {16u, 128u}) {
            flux::RenderParams q = p;
            q.max_depth = 5;
            q.nsamp = root * root;
            q.num_rows = q.img_h;
            q.fsph32 = h.filter32 ? &placeholder : nullptr;
            const flux::LaunchPlan L = flux::plan_render(q, FLUX_KERNEL_DEFAULT, FLUX_MATH_FAST);
            std::printf("plan root=%u kernel=%d typ=%d max32=%d hq_cap=%d hq_bits=%d lds=%zu K=%u\n", root, L.kernel, L.typ, L.max32, L.hq_cap,
                        L.hq_bits, L.lds, L.waves_per_pixel);
            const size_t scene_lds = 20 * sizeof(flux::DevHitRec) + sizeof(flux::DevScanSphere);
            CHECK(L.kernel == 2 && L.typ == 0 && L.max32 == 1 && L.copy == flux::kCopyFast);
            if (root == 16u) {
                CHECK(L.waves_per_pixel == 1 && L.hq_cap == 0 && L.lds == (size_t)flux::kQueueBytesPerWave + scene_lds);
            } else {
                CHECK(L.waves_per_pixel == 4 && L.hq_cap >= 64 + FLUX_HITQ_MIN_TAKE && L.hq_bits == 5);
                CHECK(L.lds == (size_t)L.hq_cap * flux::kHitQBytesPerSlot * L.waves_per_pixel + scene_lds);
            }
            CHECK(flux::plan_render(q, FLUX_KERNEL_DEFAULT, FLUX_MATH_STRICT).kernel == 1);
        }
        std::printf("ok host scene build\n");
    }
    {   // a scene without boxes keeps the image it had: with n_box = 0 the layout adds nothing behind the disks
        const AbiScene demo(scene_from_yaml_file(std::string(argv[1]) + "/disk_light.yml"));
        flux::HostScene h;
        std::string err;
        CHECK(flux::build_host_scene(demo.desc, h, err) == FLUX_OK);
        const flux::FsceneLayout f = flux::fscene_layout((size_t)h.rp.n_sph, (size_t)h.rp.n_pln, (size_t)h.rp.n_dsk, 0, (size_t)h.rp.n_shapes, 800, 600);
        CHECK(h.rp.n_box == 0 && h.fs.box == h.fs.bytes && h.fs.bytes == f.bytes && h.fs.dsk == f.dsk && h.fs.s32 == f.s32);
        CHECK(h.fs.bytes == h.fs.dsk + 2 * sizeof(flux::DevScanDisk) && h.fscene.size() == h.fs.bytes);
        CHECK(flux::hit_records(h.rp) == h.rp.n_shapes);
        std::printf("ok box-free scene\n");
    }
    std::printf("all ok\n");
    return 0;
}
