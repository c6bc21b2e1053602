// The host half of context creation (flux_amd/csrc/scene_build.cpp), CPU only (tests/test_scene_build.py builds and runs it).
//   usage: scene_build_selftest <scenes dir> <out dir>
// For each scene it writes every buffer a context uploads, as <out dir>/<scene>.<buffer>.bin, and every scene-derived scalar as
// text, <out dir>/<scene>.scalars.txt: the test pins their SHA-256.  The scenes are the shipped ones loaded through the C++ host
// layer and a generated height field whose triangles need the threaded record pool and the forked BVH build.  Small inline
// scenes cover each branch of the derived flags.  It also writes <out dir>/plans.txt: the launch planner's answer (flux_plan.h
// plan_render: kernel, instantiation, block, grid, LDS) for every scene over a grid of jobs, one line each, which the test pins too,
// and <out dir>/pass_plans.txt: the same for the per-pixel passes (feature buffers, sample moments, an adaptive pass).
// The instantiation word of flux_ctx_launch_plan (flux_plan.h plan_flags) is pinned for the headline job -- demo2, 800 x 600,
// sample root 128, depth 5 -- and for box_room at depths 5 and 3.  Every plan it asks for, and every plan of a grid of synthetic jobs
// (synthetic_plans), must name a kernel instantiation that exists (flux_plan.h kernel_exists).
// Prints one "ok <name>" per passed check and "all ok" at the end; exits 1 on the first failure.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../flux_amd/csrc/flux_plan.h"
#include "../flux_amd/csrc/scene_build.h"
#include "../flux_amd/host/flux_host.hpp"

using namespace flux_host;

#define CHECK(c)                                                            \
    do {                                                                    \
        if (!(c)) {                                                         \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);      \
            return 1;                                                       \
        }                                                                   \
    } while (0)

static std::string g_out;

static bool write_file(const std::string &name, const void *data, size_t bytes) {
    FILE *f = std::fopen((g_out + "/" + name).c_str(), "wb");
    if (!f) return false;
    const bool ok = (bytes == 0 || std::fwrite(data, 1, bytes, f) == bytes);
    return std::fclose(f) == 0 && ok;
}
template <class T> static bool write_vec(const std::string &name, const std::vector<T> &v) {
    return write_file(name, v.data(), v.size() * sizeof(T));
}

// every scalar the host build decides, one "name value" line each (doubles as %a: exact)
static std::string scalars(const flux::HostScene &h) {
    const flux::RenderParams &p = h.rp;
    std::string s;
    char buf[160];
    auto d = [&](const char *n, double v) { std::snprintf(buf, sizeof(buf), "%s %a\n", n, v); s += buf; };
    auto i = [&](const char *n, long long v) { std::snprintf(buf, sizeof(buf), "%s %lld\n", n, v); s += buf; };
    d("ex", p.ex); d("ey", p.ey); d("ez", p.ez);
    d("Ux", p.Ux); d("Uy", p.Uy); d("Uz", p.Uz); d("Vx", p.Vx); d("Vy", p.Vy); d("Vz", p.Vz); d("Wx", p.Wx); d("Wy", p.Wy); d("Wz", p.Wz);
    d("aps", p.aps); d("half_w", p.half_w); d("half_h", p.half_h); d("factor", p.factor); d("focal", p.focal);
    d("lens_radius", p.lens_radius); d("bgr", p.bgr); d("bgg", p.bgg); d("bgb", p.bgb);
    i("img_w", p.img_w); i("img_h", p.img_h); i("n_shapes", p.n_shapes); i("num_sets", p.num_sets);
    i("n_mats", p.n_mats); i("n_tris", p.n_tris); i("bvh_stack", p.bvh_stack); i("bvh4_stack", p.bvh4_stack); i("mat_bits", p.mat_bits);
    for (int a = 0; a < 3; a++) { d("bvh_qmin", p.bvh_qmin[a]); d("bvh_qstep", p.bvh_qstep[a]); }
    i("n_sph", p.n_sph); i("n_pln", p.n_pln); i("n_dsk", p.n_dsk); d("bvh_mag", p.bvh_mag);
    i("set_first", p.set_first); i("set_stride", p.set_stride); i("set_count", p.set_count); i("out_by_set", p.out_by_set);
    i("slot_first", p.slot_first); i("slot_stride", p.slot_stride);
    i("glossy_long", p.glossy_long); i("self_skip", p.self_skip); i("n_uni", p.n_uni); i("uni_idx0", p.uni_idx[0]);
    i("uni_idx1", p.uni_idx[1]); i("unit_dirs", p.unit_dirs); i("env_short", p.env_short); i("pad_env", p.pad_env);
    d("env_radius", p.env_radius); d("t_min", p.t_min); d("env_deep", p.env_deep);
    d("env_px", p.env_px); d("env_py", p.env_py); d("env_pz", p.env_pz); d("env_rr", p.env_rr); d("env_eps", p.env_eps);
    i("f32_groups", p.f32_groups); i("f32_valid", p.f32_valid); d("fwx", p.fwx); d("fwy", p.fwy); d("fwz", p.fwz);
    i("has_diel", p.has_diel);
    i("filter32", h.filter32); i("f32_half", h.f32_half); i("f32_top", h.f32_top);
    i("fs.sph", (long long)h.fs.sph); i("fs.pln", (long long)h.fs.pln); i("fs.rec", (long long)h.fs.rec); i("fs.s32", (long long)h.fs.s32);
    i("fs.ss", (long long)h.fs.ss); i("fs.pxc", (long long)h.fs.pxc); i("fs.dsk", (long long)h.fs.dsk); i("fs.bytes", (long long)h.fs.bytes);
    const flux::BvhInfo &b = h.bvh;
    i("bvh.nodes", (long long)b.nodes); i("bvh.tris", (long long)b.tris); i("bvh.max_depth", (long long)b.max_depth);
    i("bvh.max_leaf", (long long)b.max_leaf); d("bvh.mag", b.mag); i("bvh.wide_nodes", (long long)b.wide_nodes);
    i("bvh.leaf_records", (long long)b.leaf_records); i("bvh.fused_leaves", (long long)b.fused_leaves);
    i("bvh.wide_stack", (long long)b.wide_stack); d("bvh.pad", b.pad); i("bvh.arena_units", (long long)b.arena_units);
    i("bvh.split_leaves", (long long)b.split_leaves);
    return s;
}

// the FAST scene image's regions: in order, each one's records inside it, 128-B aligned where the layout says so
static bool layout_ok(const flux::HostScene &h) {
    const flux::FsceneLayout &f = h.fs;
    const flux::RenderParams &p = h.rp;
    const size_t end_sph = f.sph + (size_t)(p.n_sph + 1) * sizeof(flux::DevScanSphere);
    const size_t end_pln = f.pln + (size_t)(p.n_pln + 1) * sizeof(flux::DevScanPlane);
    const size_t end_rec = f.rec + (size_t)(p.n_shapes + 1) * sizeof(flux::DevHitRec);
    const size_t end_s32 = f.s32 + (size_t)((p.n_sph + 1) / 2 + 4) * sizeof(flux::DevScanSphere32);
    const size_t end_ss = f.ss + (size_t)(p.n_sph + 1) * sizeof(flux::DevShape);
    const size_t end_pxc = f.pxc + ((size_t)p.img_w + p.img_h) * sizeof(double);
    const size_t end_dsk = f.dsk + (size_t)(p.n_dsk + 1) * sizeof(flux::DevScanDisk);
    return f.sph == 0 && end_sph <= f.pln && end_pln <= f.rec && end_rec <= f.s32 && end_s32 <= f.ss && end_ss <= f.pxc &&
           end_pxc <= f.dsk && end_dsk <= f.bytes && f.bytes == h.fscene.size() && f.ss % 128 == 0 && f.pxc % 128 == 0 &&
           f.dsk % 128 == 0 && f.s32 % 32 == 0;
}

static int build(const flux_scene_desc &desc, flux::HostScene &h) {
    std::string err;
    const int rc = flux::build_host_scene(desc, h, err);
    if (rc != FLUX_OK) std::printf("build_host_scene: %d %s\n", rc, err.c_str());
    return rc;
}

// The launch plans of one scene, as a context would ask for them (abi.hip: rows_params / sets_params, then the traversal hook), over
// sample roots x kernel variants x arithmetic x traversal x a rows and a sets launch; max_trace_depth 5 (the job default).  Where the
// upload sets a pointer the planner tests, a placeholder stands in for it.
static std::string g_plans;
static int plans(const std::string &name, const flux::HostScene &h, const char *tag) {
    static const flux::DevScanSphere32 fsph32_placeholder{};
    static const flux::DevNode4Q nodes4_placeholder{};
    static const char *kVariant[] = {"default", "static", "refill", "split"};
    static const char *kTraversal[] = {"bvh", "brute", "binary"};
    char buf[400];
    for (const uint32_t root : {4u, 8u, 16u, 128u})
        for (const int variant : {FLUX_KERNEL_DEFAULT, FLUX_KERNEL_STATIC, FLUX_KERNEL_REFILL, FLUX_KERNEL_SPLIT})
            for (const int math : {FLUX_MATH_FAST, FLUX_MATH_STRICT})
                for (const int trav : {FLUX_TRAVERSE_BVH, FLUX_TRAVERSE_BRUTE, FLUX_TRAVERSE_BVH_BINARY})
                    for (const bool sets : {false, true}) {
                        flux::RenderParams p = h.rp;
                        p.max_depth = 5;
                        p.nsamp = root * root;
                        p.fsph32 = h.filter32 ? &fsph32_placeholder : nullptr;
                        p.nodes4 = h.arena.empty() ? nullptr : &nodes4_placeholder;
                        p.num_rows = p.img_h;
                        if (sets) {  // the first third of the sets, one rank's share at G = 3
                            p.set_count = (int32_t)(p.num_sets + 2) / 3;
                            p.out_by_set = 1;
                        }
                        if (trav == FLUX_TRAVERSE_BRUTE) p.bvh_stack = 0;
                        if (trav == FLUX_TRAVERSE_BVH_BINARY) p.nodes4 = nullptr;
                        const flux::LaunchPlan L = flux::plan_render(p, variant, math);
                        CHECK(flux::plan_exists(flux::kPassRender, L));  // (render.hip compiles the instantiation it names)
                        std::snprintf(buf, sizeof(buf),
                                      "%s%s root=%u variant=%s math=%s traversal=%s launch=%s kernel=%d copy=%d tris=%d typ=%d max32=%d "
                                      "lds_scene=%d hq_cap=%d hq_th=%d hq_bits=%d block=%u blocks=%llu lds=%zu K=%u\n",
                                      name.c_str(), tag, root, kVariant[variant], math == FLUX_MATH_STRICT ? "strict" : "fast",
                                      kTraversal[trav], sets ? "sets" : "rows", L.kernel, L.copy, L.tris, L.typ, L.max32, L.lds_scene,
                                      L.hq_cap, L.hq_th, L.hq_bits, L.block, (unsigned long long)L.blocks, L.lds, L.waves_per_pixel);
                        g_plans += buf;
                    }
    return 0;
}

// The plans of the per-pixel passes (flux_plan.h plan_pass) of one scene, for <out dir>/pass_plans.txt: sample roots
// below, at and above one wave x arithmetic x traversal x pass -- the adaptive pass over a one-entry list and over a seventh of
// the frame.  The jobs' other fields as in plans().
static std::string g_pass_plans;
static int pass_plans(const std::string &name, const flux::HostScene &h) {
    static const flux::DevNode4Q nodes4_placeholder{};
    static const char *kTraversal[] = {"bvh", "brute", "binary"};
    static const char *kPass[] = {"aov", "moments", "adaptive1", "adaptive7th"};
    char buf[300];
    for (const uint32_t root : {2u, 3u, 8u, 10u, 16u})
        for (const int math : {FLUX_MATH_FAST, FLUX_MATH_STRICT})
            for (const int trav : {FLUX_TRAVERSE_BVH, FLUX_TRAVERSE_BRUTE, FLUX_TRAVERSE_BVH_BINARY})
                for (int pass = 0; pass < 4; pass++) {
                    flux::RenderParams p = h.rp;
                    p.max_depth = 5;
                    p.nsamp = root * root;
                    p.nodes4 = h.arena.empty() ? nullptr : &nodes4_placeholder;
                    p.num_rows = p.img_h;
                    if (trav == FLUX_TRAVERSE_BRUTE) p.bvh_stack = 0;
                    if (trav == FLUX_TRAVERSE_BVH_BINARY) p.nodes4 = nullptr;
                    const uint64_t npix = (uint64_t)p.num_rows * (uint64_t)p.img_w;
                    const flux::Pass which = pass == 0 ? flux::kPassAov : pass == 1 ? flux::kPassMoments : flux::kPassAdaptive;
                    const flux::LaunchPlan L = flux::plan_pass(which, p, FLUX_KERNEL_DEFAULT, math, pass < 2 ? 0 : pass == 2 ? 1 : npix / 7 + 1);
                    CHECK(flux::plan_exists(which, L));
                    std::snprintf(buf, sizeof(buf), "%s root=%u math=%s traversal=%s pass=%s copy=%d tris=%d block=%u blocks=%llu lds=%zu\n",
                                  name.c_str(), root, math == FLUX_MATH_STRICT ? "strict" : "fast", kTraversal[trav], kPass[pass], L.copy,
                                  L.tris, L.block, (unsigned long long)L.blocks, L.lds);
                    g_pass_plans += buf;
                }
    return 0;
}

// The plan's flags word (flux_plan.h plan_flags) of a full-frame FAST render of the scene at sample root 128 with the default kernel,
// as a context of that job would report it: the throughput table and the word on its products as abi.hip's upload decides them.
static int job_flags(const char *scenes, const char *name, int depth, uint32_t &flags) {
    static const flux::DevScanSphere32 fsph32_placeholder{};
    static const double tput_placeholder = 0.0;
    const AbiScene abi(scene_from_yaml_file(std::string(scenes) + "/" + name + ".yml"));
    flux::HostScene h;
    CHECK(build(abi.desc, h) == FLUX_OK);
    flux::RenderParams p = h.rp;
    p.max_depth = depth;
    p.nsamp = 128u * 128u;
    p.fsph32 = h.filter32 ? &fsph32_placeholder : nullptr;
    p.num_rows = p.img_h;
    int bits = 0;
    if (flux::tput_table_bytes(p, &bits)) {
        std::vector<double> table;
        flux::build_tput_table(h, bits, depth, table);
        p.tput_finite = flux::tput_products_finite(h, bits, depth, table) ? 1 : 0;
        p.tput = &tput_placeholder;
        p.tput_bits = bits;
    }
    flags = flux::plan_flags(p, flux::plan_render(p, FLUX_KERNEL_DEFAULT, FLUX_MATH_FAST));
    std::printf("flags %s depth %d 0x%x\n", name, depth, flags);
    return 0;
}

// The planner over jobs the shipped scenes do not reach: every answer names an instantiation render.hip compiles (flux_plan.h
// kernel_exists).  Scene-derived fields as scene_build.cpp ties them (unit_dirs, self_skip = !glossy_long), one plane, an environment
// sphere among the spheres; a mesh has a tree of 8 levels, `nodes4`: with the 4-wide one; a context that would build the throughput
// table holds it.  Also the table itself: its rows counted.
static int synthetic_plans() {
    static const flux::DevScanSphere32 fsph32_placeholder{};
    static const flux::DevNode4Q nodes4_placeholder{};
    static const double tput_placeholder = 0.0;
    unsigned long long asked = 0;
    for (const int n_sph : {0, 1, 32, 33, 64, 65})
        for (int bits = 0; bits < 256; bits++)
            for (int plane_axis = 0; plane_axis < 4; plane_axis++)
                for (const uint32_t nsamp : {16u, 64u, 256u, 16384u})
                    for (const int max_depth : {1, 5, 9}) {
                        flux::RenderParams p{};
                        p.img_w = 32;
                        p.img_h = p.num_rows = 16;
                        p.num_sets = 32;
                        p.set_count = 32;
                        p.row_stride = p.set_stride = p.slot_stride = 1;
                        p.n_mats = 2;
                        p.n_sph = n_sph;
                        p.n_pln = 1;
                        p.n_dsk = bits & 1;
                        p.n_box = bits >> 1 & 1;
                        p.has_diel = bits >> 2 & 1;
                        p.glossy_long = bits >> 3 & 1;
                        p.unit_dirs = p.self_skip = !p.glossy_long;
                        p.n_uni = 1 + (bits >> 4 & 1);
                        p.env_short = p.n_uni == 1;
                        p.fsph32 = bits >> 5 & 1 ? &fsph32_placeholder : nullptr;
                        p.n_tris = bits >> 6 & 1;
                        p.bvh_stack = p.bvh4_stack = p.n_tris ? 8 : 0;
                        p.nodes4 = bits >> 7 & 1 ? &nodes4_placeholder : nullptr;
                        p.n_shapes = flux::hit_records(p);
                        p.plane_axis = plane_axis;
                        p.nsamp = nsamp;
                        p.max_depth = max_depth;
                        int tb = 0;
                        if (flux::tput_table_bytes(p, &tb)) {
                            p.tput = &tput_placeholder;
                            p.tput_bits = tb;
                            p.tput_finite = 1;
                        }
                        for (const int math : {FLUX_MATH_FAST, FLUX_MATH_STRICT}) {
                            for (const int variant : {FLUX_KERNEL_DEFAULT, FLUX_KERNEL_STATIC, FLUX_KERNEL_REFILL, FLUX_KERNEL_SPLIT}) {
                                const flux::LaunchPlan L = flux::plan_render(p, variant, math);
                                CHECK(L.kernel >= 0 && flux::plan_exists(flux::kPassRender, L));
                                asked++;
                            }
                            for (const flux::Pass pass : {flux::kPassAov, flux::kPassMoments, flux::kPassAdaptive, flux::kPassAovChain}) {
                                const flux::LaunchPlan L = flux::plan_pass(pass, p, FLUX_KERNEL_DEFAULT, math, 7);
                                CHECK(L.kernel == 0 && flux::plan_exists(pass, L));
                                asked++;
                            }
                        }
                    }
    // The rows of the table, STATS apart.  Every copy: static and refill x TRIS, 4, and the four passes x TRIS, 8.  FAST beside them:
    // split 2 x 4 with TYP and 2 x 2 without, the binary tree's 1, the 4-wide tree's 3: 28 in all; with the dielectric lobe split 2,
    // 1 and 2: 17; STRICT 12.  (The render kernels' 33 rows twice, for STATS, the passes' 24, shade_rays_kernel x TRIS per copy and
    // the six table and probe kernels: render.hip's 102 kernels.)
    int rows[3] = {0, 0, 0};
    for (int copy = 0; copy < 3; copy++)
        for (int pass = flux::kPassRender; pass <= flux::kPassAovChain; pass++)
            for (int kernel = 0; kernel <= 4; kernel++)
                for (int a = 0; a < 32; a++)
                    for (int axis = 0; axis < 4; axis++)
                        rows[copy] += flux::kernel_exists(copy, pass, kernel, a & 1, a >> 1 & 1, a >> 2 & 1, a >> 3 & 1, axis, a >> 4 & 1);
    CHECK(rows[flux::kCopyStrict] == 12 && rows[flux::kCopyFast] == 28 && rows[flux::kCopyFastDiel] == 17);
    static_assert(!flux::kernel_exists(flux::kCopyFastDiel, flux::kPassRender, 2, 0, 1, 1, 0, 0, 0) &&
                      !flux::kernel_exists(flux::kCopyFast, flux::kPassRender, 2, 0, 0, 1, 0, 2, 0) &&
                      flux::kernel_exists(flux::kCopyFast, flux::kPassRender, 2, 0, 1, 1, 1, 3, 0),
                  "kernel_exists is a constant expression: the launchers ask it under if constexpr");
    std::printf("ok synthetic plans (%llu)\n", asked);
    return 0;
}

static int dump(const std::string &name, const flux_scene_desc &desc) {
    flux::HostScene h;
    CHECK(build(desc, h) == FLUX_OK);
    CHECK(layout_ok(h));
    std::vector<unsigned char> mats(h.mats.size() * sizeof(flux::DevMaterial) + h.wtab.size() * sizeof(double));
    std::memcpy(mats.data(), h.mats.data(), h.mats.size() * sizeof(flux::DevMaterial));
    std::memcpy(mats.data() + h.mats.size() * sizeof(flux::DevMaterial), h.wtab.data(), h.wtab.size() * sizeof(double));
    const std::string sc = scalars(h);
    CHECK(write_vec(name + ".shapes.bin", h.shapes) && write_vec(name + ".mats.bin", mats) && write_vec(name + ".fscene.bin", h.fscene) &&
          write_vec(name + ".tris.bin", h.tris) && write_vec(name + ".nodes.bin", h.nodes) && write_vec(name + ".nodesq.bin", h.nodesq) &&
          write_vec(name + ".arena.bin", h.arena) && write_file(name + ".scalars.txt", sc.data(), sc.size()));
    if (plans(name, h, "") || pass_plans(name, h)) return 1;
    setenv("FLUX_SPLIT_HITQ_CAP", "0", 1);  // the split kernel without its hit queue
    if (plans(name, h, "+hitq_cap0")) return 1;
    unsetenv("FLUX_SPLIT_HITQ_CAP");
    std::printf("ok dump %s\n", name.c_str());
    return 0;
}

// a height field of nx x nz quads (two triangles each) over [-20, 20]^2, heights from integer arithmetic only
static void height_field(int nx, int nz, std::vector<double> &v, std::vector<uint32_t> &idx) {
    for (int j = 0; j <= nz; j++)
        for (int i = 0; i <= nx; i++) {
            const unsigned hsh = (unsigned)(i * 7919 + j * 104729) % 1000u;
            v.push_back(-20.0 + 40.0 * i / nx);
            v.push_back(-1.0 + 0.001 * hsh);
            v.push_back(-20.0 + 40.0 * j / nz);
        }
    for (int j = 0; j < nz; j++)
        for (int i = 0; i < nx; i++) {
            const uint32_t a = (uint32_t)(j * (nx + 1) + i), b = a + 1, c = a + (uint32_t)(nx + 1), d = c + 1;
            idx.insert(idx.end(), {a, c, b, b, c, d});
        }
}

static const char *kHeader = R"(scene_name: t
camera_settings:
  eye: [0, 1, -9.0]
  look_at: [0, 1, 0]
  up: [0, 1, 0]
camera_data:
  zoom_factor: 1.0
  view_plane_distance: 500.0
  focal_distance: 10.0
  lens_radius: 0.0
output_settings:
  image_width: 32
  image_height: 16
  pixel_size: 0.5
background: [0, 0, 0]
shapes:
)";
static std::string sphere(double x, double y, double z, double r, bool invert, bool emissive = false) {
    char buf[512];
    std::snprintf(buf, sizeof(buf),
                  "  - Sphere:\n      center: [%.17g, %.17g, %.17g]\n      radius: %.17g\n      material:\n%s      invert: %s\n", x, y, z,
                  r,
                  emissive ? "        Emissive:\n          color: [1, 1, 1]\n          power: 1.0\n"
                           : "        Matte:\n          diffuse_color: [0.5, 0.5, 0.5]\n          ambient_color: [1, 1, 1]\n"
                             "          diffuse_coefficient: 1.0\n",
                  invert ? "true" : "false");
    return buf;
}
static std::string plane(double nx, double ny, double nz) {
    char buf[512];
    std::snprintf(buf, sizeof(buf),
                  "  - Plane:\n      point: [0, 0, 0]\n      normal: [%.17g, %.17g, %.17g]\n      material:\n        Matte:\n"
                  "          diffuse_color: [0.5, 0.5, 0.5]\n          ambient_color: [1, 1, 1]\n          diffuse_coefficient: 1.0\n",
                  nx, ny, nz);
    return buf;
}
static int inline_scene(const std::string &shapes, flux::HostScene &h) {
    const AbiScene abi(scene_from_yaml_text(kHeader + shapes));
    return build(abi.desc, h);
}

int main(int argc, char **argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s <scenes dir> <out dir>\n", argv[0]);
        return 2;
    }
    g_out = argv[2];
    unsetenv("FLUX_SPLIT_HITQ_CAP");  // the planner's test overrides: the plans below are the shipped ones
    unsetenv("FLUX_SPLIT_HITQ_TAKE_AT");
    for (const char *name : {"demo1", "demo2", "disk_light", "glass"}) {
        const AbiScene abi(scene_from_yaml_file(std::string(argv[1]) + "/" + name + ".yml"));
        if (dump(name, abi.desc)) return 1;
    }
    {   // 256 x 160 quads = 81 920 triangles beside demo1's spheres: the record pool and the forked BVH build both run
        const AbiScene abi(scene_from_yaml_file(std::string(argv[1]) + "/demo1.yml"));
        std::vector<double> v;
        std::vector<uint32_t> idx;
        height_field(256, 160, v, idx);
        flux_mesh mesh{};
        mesh.vertices = v.data();
        mesh.num_vertices = v.size() / 3;
        mesh.indices = idx.data();
        mesh.num_triangles = idx.size() / 3;
        mesh.material = abi.shapes[1].material;
        flux_scene_desc desc = abi.desc;
        desc.meshes = &mesh;
        desc.num_meshes = 1;
        CHECK(mesh.num_triangles >= 65536);
        if (dump("heightfield", desc)) return 1;
    }

    flux::HostScene h;
    CHECK(inline_scene(sphere(0, 1, 0, 1, false) + plane(0, 1, 0), h) == FLUX_OK);
    CHECK(h.rp.glossy_long == 0 && h.rp.unit_dirs == 1 && h.rp.self_skip == 1 && layout_ok(h));
    std::printf("ok unit normal\n");
    h = flux::HostScene();
    CHECK(inline_scene(sphere(0, 1, 0, 1, false) + plane(0, 2, 0), h) == FLUX_OK);
    CHECK(h.rp.glossy_long == 1 && h.rp.unit_dirs == 0 && h.rp.self_skip == 0 && layout_ok(h));
    std::printf("ok non-unit plane normal\n");
    h = flux::HostScene();
    CHECK(inline_scene(sphere(0, 1, 0, 1, false) + sphere(2000, 0, 0, 1, false), h) == FLUX_OK);
    CHECK(h.rp.glossy_long == 0 && h.rp.self_skip == 0);
    std::printf("ok sphere beyond 1e3\n");
    h = flux::HostScene();
    CHECK(inline_scene(sphere(0, 0, 0, 100, true, true) + sphere(0, 1, 0, 1, false), h) == FLUX_OK);
    CHECK(h.rp.n_uni == 1 && h.rp.uni_idx[0] == 0 && h.rp.env_short == 1 && h.rp.env_radius >= 100.0 && h.rp.env_rr == 1e4);
    std::printf("ok one emissive invert sphere\n");
    h = flux::HostScene();
    CHECK(inline_scene(sphere(0, 1, 0, 1, false) + sphere(0, 0, 0, 100, true, true) + sphere(0, 0, 0, 200, true), h) == FLUX_OK);
    CHECK(h.rp.n_uni == 2 && h.rp.uni_idx[0] == 1 && h.rp.uni_idx[1] == 2 && h.rp.env_short == 0 && h.rp.env_radius == 0.0);
    std::printf("ok two invert spheres\n");
    {
        std::string s;
        for (int k = 0; k < 5; k++) s += sphere(3.0 * k, 1, 0, 1, false);
        h = flux::HostScene();
        CHECK(inline_scene(s, h) == FLUX_OK);
        // 5 spheres = 3 pairs: one full group of four pairs, its fourth pair padding
        CHECK(h.filter32 && h.rp.f32_valid == 0x1fu && h.rp.f32_groups == 1 && h.f32_half == -1 && h.f32_top == 4);
        s.clear();
        for (int k = 0; k < 10; k++) s += sphere(3.0 * k, 1, 0, 1, false);
        h = flux::HostScene();
        CHECK(inline_scene(s, h) == FLUX_OK);
        // 10 spheres = 5 pairs: one group, then a half group of one pair
        CHECK(h.rp.f32_valid == 0x3ffu && h.rp.f32_groups == 1 && h.f32_half == 4 && h.f32_top == 4);
        s.clear();
        for (int k = 0; k < 33; k++) s += sphere(3.0 * k, 1, 0, 1, false);
        h = flux::HostScene();
        CHECK(inline_scene(s, h) == FLUX_OK);
        CHECK(h.filter32 && h.rp.n_sph == 33 && h.rp.f32_valid == 0xffffffffu && h.rp.f32_groups == 0 && h.f32_half == -1 &&
              h.f32_top == 0 && layout_ok(h));
    }
    std::printf("ok group walk\n");
    h = flux::HostScene();
    CHECK(inline_scene(sphere(0, 0, 0, 100, true, true) + sphere(1e16, 1, 0, 1, false), h) == FLUX_OK);
    CHECK(!h.filter32 && h.rp.n_uni == 0 && h.rp.env_short == 0 && h.rp.f32_groups == 0 && h.f32_half == -1 && h.f32_top == 0);
    std::printf("ok no f32 filter\n");
    CHECK(write_file("plans.txt", g_plans.data(), g_plans.size()));
    CHECK(write_file("pass_plans.txt", g_pass_plans.data(), g_pass_plans.size()));
    std::printf("ok plans\n");
    if (synthetic_plans()) return 1;
    {
        const uint32_t fast = 1u << FLUX_PLAN_FLAG_COPY_SHIFT;
        const uint32_t hitq = FLUX_PLAN_FLAG_HITQ | FLUX_PLAN_FLAG_UNIFORM_A | FLUX_PLAN_FLAG_MAX32 | fast;
        const uint32_t table_cut = FLUX_PLAN_FLAG_TPUT_TABLE | FLUX_PLAN_FLAG_DEPTH_CUT;
        uint32_t f = 0;
        // the headline: TYP with MAX32, the hit queue with 4 bits an entry, the table, the cut, the uniform phase-A step, the floor's axis y
        if (job_flags(argv[1], "demo2", 5, f)) return 1;
        CHECK(f == (FLUX_PLAN_FLAG_TYP | hitq | table_cut | 2u << FLUX_PLAN_FLAG_AXIS_SHIFT | 4u << FLUX_PLAN_FLAG_HQ_BITS_SHIFT));
        // box_room's 17 records, 5 bits an entry: at depth 5 no table (48 MiB) and so no cut, at depth 3 both; boxes: never TYP
        if (job_flags(argv[1], "box_room", 5, f)) return 1;
        CHECK(f == (hitq | 5u << FLUX_PLAN_FLAG_HQ_BITS_SHIFT));
        if (job_flags(argv[1], "box_room", 3, f)) return 1;
        CHECK(f == (hitq | table_cut | 5u << FLUX_PLAN_FLAG_HQ_BITS_SHIFT));
        std::printf("ok flags\n");
    }
    std::printf("all ok\n");
    return 0;
}
