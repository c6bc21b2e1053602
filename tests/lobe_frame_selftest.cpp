// Which hit records get an entry of the split kernel's lobe-frame table, and how large the table is, on the CPU
// (scene_build.cpp lobe_frame_table; tests/test_lobe_frames.py builds and runs it, once more under AddressSanitizer and UBSan).
//   usage: lobe_frame_selftest <scenes dir>
// 1. demo2: the one plane's record has an entry, no sphere's has.
// 2. disk_light: the plane's and the disk's records, behind the spheres in scan order.
// 3. box_room: all six face records of each box, the disk's, and not the sphere's.
// In each scene the flags are compared with the records' own shape kinds and with the shapes counted in the YAML, the list has one
// flag per hit record, and the table's size is 48 B per record -- entries or not.
// 4. FLUX_LOBE_FRAMES=0 yields no table: size 0, an empty list; any other value, or none, yields the table.
// Prints one "ok <name>" per passed check and "all ok" at the end; exits 1 on the first failure.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <variant>
#include <vector>

#include "../flux_amd/csrc/scene_build.h"
#include "../flux_amd/host/flux_host.hpp"

using namespace flux_host;
using namespace flux;

#define CHECK(c)                                                            \
    do {                                                                    \
        if (!(c)) {                                                         \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);      \
            return 1;                                                       \
        }                                                                   \
    } while (0)

static int build(const SceneData &sd, HostScene &h) {
    const AbiScene abi(sd);
    std::string err;
    CHECK(build_host_scene(abi.desc, h, err) == FLUX_OK);
    return 0;
}

// the scene's table against its YAML: n_sph spheres first (no entry), then one record per plane and disk and six per box (entries)
static int check_scene(const std::string &path, int want_planes, int want_disks, int want_boxes) {
    const SceneData sd = scene_from_yaml_file(path);
    int sph = 0, pln = 0, dsk = 0, box = 0;
    for (const ShapeData &s : sd.shapes) {
        sph += std::holds_alternative<SphereData>(s);
        pln += std::holds_alternative<PlaneData>(s);
        dsk += std::holds_alternative<DiskData>(s);
        box += std::holds_alternative<BoxData>(s);
    }
    CHECK(pln == want_planes && dsk == want_disks && box == want_boxes);
    HostScene h;
    if (build(sd, h)) return 1;
    const int n_rec = hit_records(h.rp);
    CHECK(n_rec == sph + pln + dsk + 6 * box);
    std::vector<unsigned char> has{7, 7, 7};  // (stale content must go)
    const size_t bytes = lobe_frame_table(h, has);
    CHECK(kLobeFrameBytes == 48 && bytes == (size_t)n_rec * 48 && has.size() == (size_t)n_rec);
    const DevHitRec *rec = reinterpret_cast<const DevHitRec *>(h.fscene.data() + h.fs.rec);
    int entries = 0;
    for (int k = 0; k < n_rec; k++) {
        CHECK(has[k] == (k >= sph ? 1 : 0));  // scan order: the spheres first
        CHECK(has[k] == (rec[k].shape_kind != kShapeSphere ? 1 : 0));
        entries += has[k];
    }
    CHECK(entries == pln + dsk + 6 * box);
    // a box: six consecutive records, every one a face -- a plane's record with a stored axis normal
    for (int j = 0; j < box; j++)
        for (int f = 0; f < 6; f++) {
            const DevHitRec &R = rec[sph + pln + dsk + 6 * j + f];
            CHECK(has[sph + pln + dsk + 6 * j + f] == 1 && R.shape_kind == kShapePlane);
            CHECK(std::fabs(R.cx) + std::fabs(R.cy) + std::fabs(R.cz) == 1.0);
        }
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <scenes dir>\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    unsetenv("FLUX_LOBE_FRAMES");

    if (check_scene(dir + "/demo2.yml", 1, 0, 0)) return 1;
    std::printf("ok demo2\n");
    if (check_scene(dir + "/disk_light.yml", 1, 1, 0)) return 1;
    std::printf("ok disk\n");
    if (check_scene(dir + "/box_room.yml", 0, 1, 3)) return 1;
    std::printf("ok box\n");

    {
        HostScene h;
        if (build(scene_from_yaml_file(dir + "/demo2.yml"), h)) return 1;
        std::vector<unsigned char> has;
        setenv("FLUX_LOBE_FRAMES", "0", 1);
        has.assign(5, 1);
        CHECK(lobe_frame_table(h, has) == 0 && has.empty());
        setenv("FLUX_LOBE_FRAMES", "1", 1);
        CHECK(lobe_frame_table(h, has) == (size_t)hit_records(h.rp) * kLobeFrameBytes && has.size() == (size_t)hit_records(h.rp));
        unsetenv("FLUX_LOBE_FRAMES");
        CHECK(lobe_frame_table(h, has) == (size_t)hit_records(h.rp) * kLobeFrameBytes);
        std::printf("ok switch\n");
    }
    std::printf("all ok\n");
    return 0;
}
