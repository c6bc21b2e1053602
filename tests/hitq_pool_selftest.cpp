// The split kernel's hit queue on the CPU (tests/test_hitq_pool.py builds and runs it).
//   usage: hitq_pool_selftest <scenes dir>
// 1. The launch planner's answer for the five shipped scenes at 256 and 16384 spp, one "plan ..." line each: the test pins the pool's
//    bytes, the hit-queue / ray-queue decision and the reported fields.
// 2. The pool's arithmetic (flux_plan.h: hitq_entry_dword, hitq_admits_phase_a -- the functions the kernel's pass loop calls) for every
//    pool size from the floor to the cap: entries lie inside the pool and clear of each other, and phase A is never admitted with
//    less than 64 * 68 B free.
// Prints one "ok <name>" per passed check and "all ok" at the end; exits 1 on the first failure.
#include <cstdio>
#include <cstdlib>
#include <string>

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

static int plan_lines(const std::string &dir, const char *name) {
    const AbiScene abi(scene_from_yaml_file(dir + "/" + name + ".yml"));
    HostScene h;
    std::string err;
    CHECK(build_host_scene(abi.desc, h, err) == FLUX_OK);
    static const DevScanSphere32 fsph32_placeholder{};
    for (const uint32_t root : {16u, 128u}) {
        RenderParams p = h.rp;
        p.max_depth = 5;
        p.nsamp = root * root;
        p.fsph32 = h.filter32 ? &fsph32_placeholder : nullptr;
        p.num_rows = p.img_h;
        const LaunchPlan L = plan_render(p, FLUX_KERNEL_DEFAULT, FLUX_MATH_FAST);
        const size_t scene_lds = (size_t)hit_records(p) * sizeof(DevHitRec) + (size_t)p.n_sph * sizeof(DevScanSphere);
        std::printf("plan %s root=%u kernel=%d typ=%d hq_cap=%d hq_th=%d hq_bits=%d K=%u lds=%zu queue_bytes_per_wave=%zu\n", name, root, L.kernel,
                    L.typ, L.hq_cap, L.hq_th, L.hq_bits, L.waves_per_pixel, L.lds, (L.lds - scene_lds) / L.waves_per_pixel);
        // a plan with the hit queue reserves C slots of 68 B a wave, and at least the floor
        if (L.hq_cap) CHECK(L.lds == (size_t)L.hq_cap * kHitQBytesPerSlot * L.waves_per_pixel + scene_lds && L.hq_cap >= 64 + L.hq_th);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <scenes dir>\n", argv[0]);
        return 2;
    }
    unsetenv("FLUX_SPLIT_HITQ_CAP");
    unsetenv("FLUX_SPLIT_HITQ_TAKE_AT");
    for (const char *name : {"demo1", "demo2", "disk_light", "box_room", "glass"})
        if (plan_lines(argv[1], name)) return 1;
    std::printf("ok plans\n");

    static_assert(kHitQDwordsPerSlot * 4 == kHitQBytesPerSlot && kHitQBytesPerSlot == 68, "the slot");
    static_assert(kHitQDwordsPerSlot % 2 == 1, "an odd stride: a wave's accesses do not collide on LDS banks");
    // every pool size from the floor (64 + H slots, H from 1) to past demo2's 110: entry k of n parked ones lies inside the pool's
    // C * 68 bytes, below entry k - 1 and clear of it, and phase A is admitted only with 64 * 68 B free -- room for the 64 entries
    // its scan may park, which then still lie inside the pool
    for (uint32_t C = 65; C <= 128; ++C)
        for (uint32_t n = 0; n <= C; ++n) {
            if (n) {
                const uint32_t at = hitq_entry_dword(C, n - 1u);
                CHECK(at + kHitQDwordsPerSlot <= C * kHitQDwordsPerSlot);
                CHECK(n < 2u || at + kHitQDwordsPerSlot == hitq_entry_dword(C, n - 2u));
            }
            const uint32_t free_bytes = (C - n) * 68u;
            CHECK(hitq_admits_phase_a(C, n) == (free_bytes >= 64u * 68u));
            if (hitq_admits_phase_a(C, n)) CHECK(hitq_entry_dword(C, n + 63u) + kHitQDwordsPerSlot <= C * kHitQDwordsPerSlot);
        }
    CHECK(hitq_entry_dword(110, 0) == 109u * 17u && hitq_entry_dword(110, 109) == 0u);
    std::printf("ok room test\n");
    std::printf("all ok\n");
    return 0;
}
