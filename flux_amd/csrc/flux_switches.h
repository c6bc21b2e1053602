// flux_switches.h -- every environment variable the library reads, and the only place it calls getenv.
//
// The switches keep an older path reachable for tests and A/B runs; none is part of the C ABI.  Nothing is cached: a switch is read
// where the column "read" says, every time, so a test may flip one on a live context (DESIGN.md "Environment switches" holds the
// same rows).  An on/off switch is OFF when it is set and atoi() of it is 0 ("0", "", "abc"); unset, "1", "-3" and "7x" leave it on.
//
// variable                 default                                     a value                                      read                      pinned by (tests/)
// FLUX_SAMPLE_TABLES       glossy-lobe angle table (glossx) built      off: every glossy bounce does the arithmetic during flux_ctx_create*   test_gpu_sample_tables.py
// FLUX_THROUGHPUT_TABLE    throughput product table uploaded           off: the take multiplies the list up         during flux_ctx_create*   test_gpu_throughput_table.py
// FLUX_LOBE_FRAMES         lobe-frame table, 48 B per hit record       off: every bounce builds its frame           during flux_ctx_create*   test_gpu_lobe_frames.py, test_lobe_frames.py
// FLUX_PLANE_AXIS          first plane's axis stated to the scans      off: both scans form its dot products        during flux_ctx_create*   test_gpu_plane_axis.py
// FLUX_SAMPLE_ORDER        samples in first-bounce direction order     off: the identity order                      during flux_ctx_create*   test_gpu_sample_order.py
// FLUX_SPLIT_DEPTH_CUT     a path ends at the depth limit              off: no cut in either loop                   every planner call        test_gpu_depth_cut.py, test_depth_cut.py
// FLUX_SPLIT_UNIFORM_A     one-shape waves shaded from scalars         off: phase A's general step for every wave   every planner call        test_gpu_uniform_phase_a.py
// FLUX_SPLIT_HITQ_CAP      hit queue of as many slots as the LDS fits  min(that, max(0, atoi) & ~1u) slots; 0: none every planner call        test_gpu_split_hit_queue.py, test_scene_build.py
// FLUX_SPLIT_HITQ_TAKE_AT  H = min(64, cap - 64), at least the minimum clamp(atoi, 1, 64) replaces H                every planner call        test_gpu_hitq_classes.py, test_hitq_pool.py
// FLUX_DENOISE_LDS_LEVELS  kDefaultLdsLevels levels filter from LDS    atoi replaces it                             every denoise launch      denoise_checks.py
// FLUX_BUILD_THREADS       hardware_concurrency, clamped to 1..16      max(1, atoi), clamped to 1..16               every mesh / BVH build    test_scene_build.py, test_bvh_builder.py
// FLUX_RCCL_LIB            the process's or the loader's librccl       a path, tried first                          first RCCL load           (none)
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <optional>
#include <thread>

namespace flux {

constexpr const char *kEnvSampleTables = "FLUX_SAMPLE_TABLES";
constexpr const char *kEnvThroughputTable = "FLUX_THROUGHPUT_TABLE";
constexpr const char *kEnvLobeFrames = "FLUX_LOBE_FRAMES";
constexpr const char *kEnvPlaneAxis = "FLUX_PLANE_AXIS";
constexpr const char *kEnvSampleOrder = "FLUX_SAMPLE_ORDER";
constexpr const char *kEnvSplitDepthCut = "FLUX_SPLIT_DEPTH_CUT";
constexpr const char *kEnvSplitUniformA = "FLUX_SPLIT_UNIFORM_A";

// An on/off switch: off when set and atoi() == 0
inline bool switch_off(const char *name) {
    const char *e = std::getenv(name);
    return e && std::atoi(e) == 0;
}

// A numeric switch: atoi() of it when set
inline std::optional<int> switch_int(const char *name) {
    const char *e = std::getenv(name);
    return e ? std::optional<int>(std::atoi(e)) : std::nullopt;
}

// The hit queue's slots, of the `cap` that fit
inline uint32_t hitq_cap(uint32_t cap) {
    const std::optional<int> v = switch_int("FLUX_SPLIT_HITQ_CAP");
    return v ? std::min(cap, (uint32_t)std::max(0, *v) & ~1u) : cap;
}

// H, the parked hits at which a wave takes a batch
inline uint32_t hitq_take_at(uint32_t th) {
    const std::optional<int> v = switch_int("FLUX_SPLIT_HITQ_TAKE_AT");
    return v ? (uint32_t)std::max(1, std::min(64, *v)) : th;
}

inline int denoise_lds_levels(int dflt) { return switch_int("FLUX_DENOISE_LDS_LEVELS").value_or(dflt); }

// The threads of a mesh or BVH build: 1..16
inline unsigned build_threads() {
    unsigned threads = std::thread::hardware_concurrency();
    if (const std::optional<int> v = switch_int("FLUX_BUILD_THREADS")) threads = (unsigned)std::max(1, *v);
    return std::min(std::max(threads, 1u), 16u);
}

inline const char *rccl_lib() { return std::getenv("FLUX_RCCL_LIB"); }

}  // namespace flux
