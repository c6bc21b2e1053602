// When the split kernel's depth cut is admitted (launch_plan.cpp split_cut_depth, scene_build.cpp tput_products_finite), on the CPU
// (tests/test_depth_cut.py builds and runs it, once more under AddressSanitizer and UBSan).
//   usage: depth_cut_selftest <scenes dir>
// 1. Finite tables: demo2's and a 16-record scene's at depth 5, demo2's at depths 2 and 3 -- every product finite.
// 2. Tables that are not: demo2's with one entry made infinite, with one made NaN; a floor of colour 1e200 (its lists of two entries
//    overflow); weights of 1e70 at depth 5 -- every ENTRY finite (1e280), the bounce at the depth limit not (1e350): refused too;
//    the same weights at depth 4 are admitted (1e280 is the largest product there).  A table of the wrong size, and depth 1, are refused.
// 3. The plan: a job with the hit queue gets cut_depth = max_depth exactly when the context found its products finite
//    (RenderParams::tput_finite), with or without the device's copy of the table; a job that gets no table -- depth 1 -- keeps
//    kNoDepthCut; a job with the ray queue (demo2 at 256 spp, glass) gets max_depth unconditionally; FLUX_SPLIT_DEPTH_CUT=0 turns
//    every one of them off, FLUX_SPLIT_DEPTH_CUT=1 none.
// Prints one "ok <name>" per passed check and "all ok" at the end; exits 1 on the first failure.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "../flux_amd/csrc/flux_plan.h"
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

static const DevScanSphere32 fsph32_placeholder{};
static const double tput_placeholder[3] = {0.0, 0.0, 0.0};  // (a device table's address: the planner never reads through it)

// the job's RenderParams as the upload fills them, as far as the planner reads them
static RenderParams job_params(const HostScene &h, uint32_t root, int depth) {
    RenderParams p = h.rp;
    p.max_depth = depth;
    p.nsamp = root * root;
    p.fsph32 = h.filter32 ? &fsph32_placeholder : nullptr;
    p.num_rows = p.img_h;
    return p;
}

static int build(const SceneData &sd, HostScene &h) {
    const AbiScene abi(sd);
    std::string err;
    CHECK(build_host_scene(abi.desc, h, err) == FLUX_OK);
    return 0;
}

// `sd` with Matte planes below the floor added until the scene has `records` hit records
static SceneData padded(SceneData sd, int records) {
    HostScene h;
    if (build(sd, h)) std::exit(1);
    for (int k = 0; hit_records(h.rp) + k < records; k++) {
        MatteData m;
        m.diffuse_color = Color{0.11 + 0.07 * k, 0.93 - 0.05 * k, 0.31 + 0.013 * k};
        m.diffuse_coefficient = 0.61 + 0.03 * k;
        sd.shapes.push_back(PlaneData{Vec3{0.0, -50.0 - k, 0.0}, Vec3{0.0, 1.0, 0.0}, m});
    }
    return sd;
}

// `sd` with one more Matte plane whose bounce weight is `w` in every channel
static SceneData with_weight(SceneData sd, double w) {
    MatteData m;
    m.diffuse_color = Color{w, w, w};
    m.diffuse_coefficient = 1.0;
    sd.shapes.push_back(PlaneData{Vec3{0.0, -60.0, 0.0}, Vec3{0.0, 1.0, 0.0}, m});
    return sd;
}

static int table_of(const HostScene &h, int depth, int &bits, std::vector<double> &tab) {
    CHECK(tput_table_bytes(job_params(h, 128, depth), &bits) != 0);
    build_tput_table(h, bits, depth, tab);
    return 0;
}

static int cut_of(RenderParams p) { return plan_render(p, FLUX_KERNEL_SPLIT, FLUX_MATH_FAST).cut_depth; }

int main(int argc, char **argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <scenes dir>\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    unsetenv("FLUX_SPLIT_HITQ_CAP");
    unsetenv("FLUX_SPLIT_HITQ_TAKE_AT");
    unsetenv("FLUX_SPLIT_DEPTH_CUT");
    static_assert(kNoDepthCut == 0x7ffffffe, "above every depth limit, below the kernel's mark of a lane without a path");

    const SceneData demo2 = scene_from_yaml_file(dir + "/demo2.yml");
    HostScene h2, h16, hbig, h70, glass;
    if (build(demo2, h2) || build(padded(demo2, 16), h16) || build(with_weight(demo2, 1e200), hbig) || build(with_weight(demo2, 1e70), h70) ||
        build(scene_from_yaml_file(dir + "/glass.yml"), glass))
        return 1;
    int bits = 0;
    std::vector<double> tab;

    for (const int depth : {5, 3, 2}) {
        if (table_of(h2, depth, bits, tab)) return 1;
        CHECK(tput_products_finite(h2, bits, depth, tab));
    }
    if (table_of(h16, 5, bits, tab)) return 1;
    CHECK(hit_records(h16.rp) == 16 && tput_products_finite(h16, bits, 5, tab));
    std::printf("ok finite tables\n");

    {
        if (table_of(h2, 5, bits, tab)) return 1;
        const size_t a_list = (size_t)tput_index(2u * (uint32_t)bits, 0x21u) * 3 + 1, another = (size_t)tput_index(4u * (uint32_t)bits, 0x3210u) * 3;
        std::vector<double> bad = tab;
        bad[a_list] = std::numeric_limits<double>::infinity();
        CHECK(!tput_products_finite(h2, bits, 5, bad));
        bad = tab;
        bad[another] = std::numeric_limits<double>::quiet_NaN();
        CHECK(!tput_products_finite(h2, bits, 5, bad));
        bad = tab;
        bad[a_list] = -std::numeric_limits<double>::infinity();
        bad[another] = std::numeric_limits<double>::quiet_NaN();
        CHECK(!tput_products_finite(h2, bits, 5, bad));
        bad = tab;
        bad.pop_back();
        CHECK(!tput_products_finite(h2, bits, 5, bad));  // not this job's table
        CHECK(!tput_products_finite(h2, bits, 1, std::vector<double>()));  // depth 1: no parked hit, no table
        CHECK(tput_products_finite(h2, bits, 5, tab));

        std::vector<double> big;
        if (table_of(hbig, 5, bits, big)) return 1;
        CHECK(!tput_products_finite(hbig, bits, 5, big));
        if (table_of(hbig, 2, bits, big)) return 1;  // lists of one entry (1e200), and 1e200 * 1e200 at the limit
        CHECK(!tput_products_finite(hbig, bits, 2, big));

        std::vector<double> t70;
        if (table_of(h70, 5, bits, t70)) return 1;
        bool entries_finite = true;
        double largest = 0.0;
        for (const double v : t70) {
            entries_finite = entries_finite && std::isfinite(v);
            largest = std::fmax(largest, std::fabs(v));
        }
        CHECK(entries_finite && largest > 1e279 && largest < 1e281);  // 1e70^4
        CHECK(!tput_products_finite(h70, bits, 5, t70));              // 1e70^5
        if (table_of(h70, 4, bits, t70)) return 1;
        CHECK(tput_products_finite(h70, bits, 4, t70));               // 1e70^4 at the limit
        std::printf("ok tables that are not finite\n");
    }

    for (const char *env : {(const char *)nullptr, "1", "0"}) {
        if (env) setenv("FLUX_SPLIT_DEPTH_CUT", env, 1);
        const bool on = !(env && env[0] == '0');
        // the hit queue: demo2 and the 16-record scene at 16384 spp, depth 5
        for (const HostScene *h : {&h2, &h16}) {
            RenderParams p = job_params(*h, 128, 5);
            const LaunchPlan L = plan_render(p, FLUX_KERNEL_SPLIT, FLUX_MATH_FAST);
            CHECK(L.kernel == 2 && L.hq_cap > 0 && L.hq_bits == 4);
            CHECK(L.cut_depth == kNoDepthCut);  // nobody vouches for the products
            p.tput_finite = 1;
            CHECK(cut_of(p) == (on ? 5 : kNoDepthCut));  // the context's word alone: its device may hold no copy of the table
            CHECK(split_cut_depth(p, L) == (on ? 5 : kNoDepthCut));
            p.tput = tput_placeholder;
            p.tput_bits = L.hq_bits;
            CHECK(cut_of(p) == (on ? 5 : kNoDepthCut));
            p.tput_finite = 0;  // a table whose products are not all finite
            CHECK(cut_of(p) == kNoDepthCut);
        }
        {   // depth 1: the hit queue is planned, a table never exists
            RenderParams p = job_params(h2, 128, 1);
            CHECK(plan_render(p, FLUX_KERNEL_SPLIT, FLUX_MATH_FAST).hq_cap > 0 && tput_table_bytes(p) == 0 && cut_of(p) == kNoDepthCut);
        }
        // the ray queue: no table, no condition
        for (const int depth : {1, 2, 5}) {
            const RenderParams p = job_params(h2, 16, depth), g = job_params(glass, 128, depth);
            CHECK(plan_render(p, FLUX_KERNEL_SPLIT, FLUX_MATH_FAST).hq_cap == 0 && cut_of(p) == (on ? depth : kNoDepthCut));
            CHECK(plan_render(g, FLUX_KERNEL_SPLIT, FLUX_MATH_FAST).hq_cap == 0 && cut_of(g) == (on ? depth : kNoDepthCut));
        }
        // other kernels' plans carry none
        CHECK(plan_render(job_params(h2, 128, 5), FLUX_KERNEL_REFILL, FLUX_MATH_FAST).cut_depth == kNoDepthCut);
    }
    unsetenv("FLUX_SPLIT_DEPTH_CUT");
    std::printf("ok plan\n");
    std::printf("all ok\n");
    return 0;
}
