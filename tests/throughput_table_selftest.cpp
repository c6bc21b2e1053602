// The split kernel's throughput product table and its hit-queue slot on the CPU (tests/test_throughput_table.py builds and runs it,
// once more under AddressSanitizer and UBSan).
//   usage: throughput_table_selftest <scenes dir>
// 1. The slot (flux_plan.h HitQField): the seven doubles on even dwords, the three ints in dwords 14-16, 17 dwords in all.
// 2. The index (flux_plan.h tput_index) of (n, ml) for lists of n = 1 .. 4 entries: inside the table, no two lists on one entry.
// 3. For demo2 and for a scene of 16 hit records at depth 5: every entry of build_tput_table equals, as a bit pattern, the product
//    the kernel's loop forms for that list -- the first bounce's weight, then one multiplication per bounce, front to back -- and
//    every other entry is zero.
// 4. The launch planner's answer for the shipped scenes at 256 and 16384 spp, one "plan ..." line each (the test pins every field).
// 5. Which jobs get a table: demo2 and the 16-record scene at depth 5 do (3 MiB); a scene of 17 records at depth 5, demo2 at depth 9,
//    demo2 at 256 spp (no hit queue), depth 1 (no parked hit) and glass (a dielectric: the ray queue) do not.
// Prints one "ok <name>" per passed check and "all ok" at the end; exits 1 on the first failure.
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

// `sd` with Matte planes added, each with a colour of its own, until the scene has `records` hit records
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

static int plan_lines(const std::string &dir, const char *name) {
    HostScene h;
    if (build(scene_from_yaml_file(dir + "/" + name + ".yml"), h)) return 1;
    for (const uint32_t root : {16u, 128u}) {
        const LaunchPlan L = plan_render(job_params(h, root, 5), FLUX_KERNEL_DEFAULT, FLUX_MATH_FAST);
        std::printf("plan %s root=%u kernel=%d block=%u blocks=%llu lds=%zu K=%u hq_cap=%d hq_th=%d hq_bits=%d typ=%d max32=%d\n", name, root,
                    L.kernel, L.block, (unsigned long long)L.blocks, L.lds, L.waves_per_pixel, L.hq_cap, L.hq_th, L.hq_bits, L.typ, L.max32);
    }
    return 0;
}

// every entry of the scene's table against the kernel's loop (render_body.inc render_split_kernel, the take without a table)
static int table_equals_the_loop(const HostScene &h, int records, int depth) {
    int bits = 0;
    const size_t bytes = tput_table_bytes(job_params(h, 128, depth), &bits);
    CHECK(hit_records(h.rp) == records && bytes == ((size_t)2 << (bits * (depth - 1))) * kTputEntryBytes && bytes <= kTputTableMaxBytes);
    CHECK((1 << bits) >= records && (1 << (bits - 1)) < records);
    std::vector<double> tab;
    build_tput_table(h, bits, depth, tab);
    CHECK(tab.size() * sizeof(double) == bytes);
    const DevHitRec *recs = reinterpret_cast<const DevHitRec *>(h.fscene.data() + h.fs.rec);
    const uint32_t bmask = (1u << bits) - 1u;
    std::vector<char> seen(tab.size() / 3, 0);
    size_t lists = 0;
    for (int n = 1; n < depth; n++)
        for (uint32_t ml = 0; ml < (1u << (n * bits)); ml++) {
            bool valid = true;
            for (int k = 0; k < n; k++) valid = valid && ((ml >> (k * bits)) & bmask) < (uint32_t)records;
            if (!valid) continue;
            // (the kernel's loop: a parked hit at depth d = n + 1)
            const int d = n + 1;
            const DevHitRec &R0 = recs[ml & bmask];
            double tr = R0.fr, tg = R0.fg, tb = R0.fb;
            for (int k = 1; k < d - 1; ++k) {
                const DevHitRec &Rk = recs[(ml >> (k * bits)) & bmask];
                tr *= Rk.fr;
                tg *= Rk.fg;
                tb *= Rk.fb;
            }
            const double want[3] = {tr, tg, tb};
            const uint32_t at = tput_index((uint32_t)(n * bits), ml);
            CHECK((size_t)at < seen.size() && !seen[at]);
            seen[at] = 1;
            lists++;
            CHECK(std::memcmp(&tab[(size_t)at * 3], want, sizeof(want)) == 0);
        }
    size_t expect = 0, pw = 1;
    for (int n = 1; n < depth; n++) expect += (pw *= (size_t)records);
    CHECK(lists == expect);
    const double zero[3] = {0.0, 0.0, 0.0};
    for (size_t at = 0; at < seen.size(); at++)
        if (!seen[at]) CHECK(std::memcmp(&tab[at * 3], zero, sizeof(zero)) == 0);
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <scenes dir>\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    unsetenv("FLUX_SPLIT_HITQ_CAP");
    unsetenv("FLUX_SPLIT_HITQ_TAKE_AT");

    static_assert(kHitQOx == 0 && kHitQOy == 2 && kHitQOz == 4 && kHitQDx == 6 && kHitQDy == 8 && kHitQDz == 10 && kHitQT == 12,
                  "the doubles: dword pairs on even dwords of the slot");
    static_assert(kHitQHitDepth == 14 && kHitQSample == 15 && kHitQList == 16, "the ints behind them");
    static_assert(kHitQDoubles * 2 == kHitQHitDepth && kHitQList + 1 == kHitQDwordsPerSlot && kHitQDwordsPerSlot == 17 && kHitQBytesPerSlot == 68,
                  "seven doubles, three ints, 17 dwords");
    std::printf("ok slot\n");

    // lists of n = 1 .. 4 entries of 4 bits (demo2): the entries of length n are [2^(4n), 2^(4n+1)), inside 2 << 16 entries, and the
    // formula is the documented one
    {
        const int bits = 4;
        uint32_t prev_end = 0;
        for (int n = 1; n <= 4; n++) {
            const uint32_t lo = tput_index((uint32_t)(n * bits), 0u), hi = tput_index((uint32_t)(n * bits), (1u << (n * bits)) - 1u);
            CHECK(lo == (1u << (n * bits)) && hi == (2u << (n * bits)) - 1u && lo >= prev_end && hi < (2u << (4 * bits)));
            for (uint32_t ml = 0; ml < (1u << (n * bits)); ml += 37u) CHECK(tput_index((uint32_t)(n * bits), ml) == (lo | ml) && (lo & ml) == 0u);
            prev_end = hi + 1u;
        }
        CHECK(tput_index(4, 0xb) == 0x1b && tput_index(8, 0x3b) == 0x13b && tput_index(12, 0xa3b) == 0x1a3b && tput_index(16, 0x7a3b) == 0x17a3b);
        CHECK(((size_t)2 << 16) * kTputEntryBytes == 3145728 && kTputTableMaxBytes == 4194304 && (kTputTableMaxBytes / kTputEntryBytes) < (1u << 24));
        std::printf("ok index\n");
    }

    const SceneData demo2 = scene_from_yaml_file(dir + "/demo2.yml");
    HostScene h2, h16, h17;
    if (build(demo2, h2) || build(padded(demo2, 16), h16) || build(padded(demo2, 17), h17)) return 1;
    const int n2 = hit_records(h2.rp);
    CHECK(n2 > 8 && n2 < 16);
    if (table_equals_the_loop(h2, n2, 5) || table_equals_the_loop(h16, 16, 5)) return 1;
    // shallower jobs: lists of one and two entries only
    if (table_equals_the_loop(h2, n2, 2) || table_equals_the_loop(h2, n2, 3)) return 1;
    std::printf("ok table\n");

    for (const char *name : {"demo1", "demo2", "disk_light", "box_room", "glass"})
        if (plan_lines(dir, name)) return 1;
    std::printf("ok plans\n");

    {
        int bits = -1;
        CHECK(tput_table_bytes(job_params(h2, 128, 5), &bits) == 3145728 && bits == 4);
        CHECK(tput_table_bytes(job_params(h16, 128, 5), &bits) == 3145728 && bits == 4);
        CHECK(hit_records(h17.rp) == 17 && plan_render(job_params(h17, 128, 5), FLUX_KERNEL_DEFAULT, FLUX_MATH_FAST).hq_bits == 5);
        CHECK(tput_table_bytes(job_params(h17, 128, 5)) == 0);  // 2 << 20 entries: 48 MiB
        CHECK(tput_table_bytes(job_params(h17, 128, 3), &bits) == ((size_t)2 << 10) * kTputEntryBytes && bits == 5);
        CHECK(plan_render(job_params(h2, 128, 9), FLUX_KERNEL_DEFAULT, FLUX_MATH_FAST).hq_cap == 0 && tput_table_bytes(job_params(h2, 128, 9)) == 0);
        CHECK(plan_render(job_params(h2, 128, 8), FLUX_KERNEL_DEFAULT, FLUX_MATH_FAST).hq_cap > 0 && tput_table_bytes(job_params(h2, 128, 8)) == 0);
        CHECK(plan_render(job_params(h2, 16, 5), FLUX_KERNEL_DEFAULT, FLUX_MATH_FAST).hq_cap == 0 && tput_table_bytes(job_params(h2, 16, 5)) == 0);
        CHECK(tput_table_bytes(job_params(h2, 128, 1)) == 0);
        HostScene glass, box;
        if (build(scene_from_yaml_file(dir + "/glass.yml"), glass) || build(scene_from_yaml_file(dir + "/box_room.yml"), box)) return 1;
        CHECK(tput_table_bytes(job_params(glass, 128, 5)) == 0);
        // box_room: 5 bits an entry -- the loop at depth 5, a table at depth 3
        CHECK(tput_table_bytes(job_params(box, 128, 5)) == 0 && tput_table_bytes(job_params(box, 128, 3), &bits) == 49152 && bits == 5);
        std::printf("ok which jobs\n");
    }
    std::printf("all ok\n");
    return 0;
}
