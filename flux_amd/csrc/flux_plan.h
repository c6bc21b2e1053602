// flux_plan.h -- the launch planner (launch_plan.cpp) and what it shares with the render kernels (render.hip): the tunables that
// size a launch and the LDS layout of the split kernel's queues.  Both sides read these numbers from here, so a -D override
// (scripts/sweep_variants.py) reaches the kernels and the plan alike.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "flux_device.h"

// Block size of the static and BVH kernels: measured on demo2 at 1024 spp (refill kernel): 256 threads x 2 waves/SIMD 88.6 ms;
// 256 x 3 71.7 ms; 64 x 3 70.7 ms; 256 x 4 83.0 ms (spills).  Waves never cooperate, so one wave per block lets the LDS stack of a
// finished wave be reused at once.
#ifndef FLUX_BLOCK_THREADS
#define FLUX_BLOCK_THREADS 64
#endif
#ifndef FLUX_WPE_SPLIT
#define FLUX_WPE_SPLIT 5          // waves/SIMD of the split kernel: 96 VGPRs, nothing spilled since round 4 (4 until then: 128 VGPRs); demo2 @16384 spp 250.0 -> 225.4 ms
#endif
#ifndef FLUX_HITQ_MIN_TAKE
// H, the parked hits a wave waits for before a pass takes them instead of starting 64 more samples, is C - 64 (at most 64): phase A
// runs while the queue has room for its 64 continuations.  Below this H the bounce batches are too thin to pay for the queue
// (demo2 @16384 spp, C = 110: H 46 159.2, 40 162.9, 32 171.0, 24 182.3, 16 200.9 ms; the ray queue 172.0 ms), and the scene keeps
// the ray queue.
#define FLUX_HITQ_MIN_TAKE 32
#endif

namespace flux {

// Most distinct glossy exponents a context tabulates the lobe's angles for (RenderParams::glossx): a scene with more keeps the
// arithmetic in the loop
constexpr int kGlossExpSlots = 4;

// The split kernel's ray queue: 64 queued paths per wave, structure of arrays [field][slot]: ox oy oz dx dy dz tr tg tb, then the
// sample index and Path::self (int)
constexpr int kQueueDoubles = 9;
constexpr int kQueueBytesPerWave = (kQueueDoubles * 64) * 8 + 2 * 64 * 4;
// The hit queue (plan_render chooses C per scene): C slots per wave -- o d t, hit | depth << 16, the
// sample index and the bounce list (render_body.inc render_split_kernel): 68 B a slot
constexpr int kHitQDoubles = 7;
constexpr int kHitQInts = 3;
constexpr int kHitQBytesPerSlot = kHitQDoubles * 8 + kHitQInts * 4;
// A wave's pool is an array of C such slots, 17 dwords each (an odd stride: a wave's accesses do not collide on LDS banks): the seven
// doubles first, each a dword pair at an even dword of the slot (4-byte alignment: one ds_read2_b32 / ds_write2_b32 is one double),
// then the three ints.  Entries are allocated downwards from the pool's top: entry k (0 the oldest) is slot C - 1 - k.
enum HitQField : uint32_t {  // a field's first dword in its slot
    kHitQOx = 0, kHitQOy = 2, kHitQOz = 4, kHitQDx = 6, kHitQDy = 8, kHitQDz = 10, kHitQT = 12,
    kHitQHitDepth = 14,  // hit | depth << 16
    kHitQSample = 15,
    kHitQList = 16,      // the bounce list
};
constexpr uint32_t kHitQDwordsPerSlot = kHitQBytesPerSlot / 4;
constexpr uint32_t hitq_entry_dword(uint32_t C, uint32_t k) { return (C - 1u - k) * kHitQDwordsPerSlot; }
// The room phase A needs before it runs: the scan behind it may park a hit from each of its 64 lanes.
constexpr bool hitq_admits_phase_a(uint32_t C, uint32_t nhit) { return nhit + 64u <= C; }

// The throughput product table (RenderParams::tput): for a scene whose parked hits the hit queue takes, the
// product of the bounce weights of every bounce list a parked hit can carry, so that the take reads it instead of multiplying it up.
// A list of n entries (n = depth - 1 = 1 .. max_depth - 1, hq_bits each, entry 0 the first bounce) is entry
//     tput_index(n * hq_bits, ml) = (1 << n * hq_bits) | ml
// -- the lists of length n fill [2^(n bits), 2^(n bits + 1)), so the table has 2 << (max_depth - 1) * hq_bits entries of
// kTputEntryBytes (r, g, b).  The index relies on ml's bits above n * hq_bits being zero; they are by construction (the kernel
// sets ml = hit, then ml |= hit << n * hq_bits per bounce, hit < 2^hq_bits).
// A context holds the table only while it stays within kTputTableMaxBytes (demo2, 12 records, 4 bits, depth 5: 2^17 entries, 3 MiB;
// 17 records or more at depth 5, 5 bits: 48 MiB -- no table, the take multiplies the list up as before).
constexpr size_t kTputEntryBytes = 24;
constexpr size_t kTputTableMaxBytes = (size_t)4 << 20;
constexpr uint32_t tput_index(uint32_t list_bits, uint32_t ml) { return (1u << list_bits) | ml; }
// Bytes of the table a context for this job builds -- rp as the upload fills it: the scene's fields, nsamp and max_depth --, 0 for
// none: the hit queue is not planned for the job (launch_plan.cpp plan_render), a parked hit cannot exist (max_depth < 2), or the table
// would exceed the cap.  `bits`: the hit queue's bits per list entry the table is laid out for.
size_t tput_table_bytes(const RenderParams &p, int *bits = nullptr);

// "No depth cut" as the split kernel's cut depth: a depth no live path holds -- above every depth limit, below the 0x7fffffff that
// marks a lane without a path (render_body.inc kDeadDepth)
constexpr int kNoDepthCut = 0x7ffffffe;

// The copy of render_body.inc a launch runs (render.hip): the STRICT arithmetic, the FAST one, or the FAST one with the dielectric
// lobe (RenderParams::has_diel)
enum KernelCopy { kCopyStrict = 0, kCopyFast = 1, kCopyFastDiel = 2 };
KernelCopy kernel_copy(const RenderParams &p, int math);

// Which kernel a render launch runs for these parameters -- which instantiation, with what block size, grid and dynamic LDS: decided
// in ONE place (launch_plan.cpp plan_render) and asked from there by the launch itself, by the host's LDS budget check and by
// flux_ctx_launch_plan / flux_ctx_bvh_info, so that they cannot drift apart.  The launch copies these fields into template and kernel
// arguments and decides nothing (render_body.inc launch_render_impl); which combinations of them are compiled: kernel_exists below.
struct LaunchPlan {
    int kernel = -1;  // FLUX_PLAN_* (include/flux_abi.h): 0 static, 1 refill, 2 split, 3 BVH state machine over the binary tree,
                      // 4 the same over the 4-wide tree; -1 nothing to do
    unsigned block = 64;
    uint64_t blocks = 0;
    size_t lds = 0;                // dynamic LDS per block (the refill / split kernels add 96 B of static LDS)
    unsigned waves_per_pixel = 1;  // K: waves that share one pixel's samples (1 in the static and BVH kernels)
    int lds_scene = 0;             // kernel 4: 1 = the instantiation that keeps the analytic set's records and the materials in LDS (`lds` includes them)
    int hq_cap = 0, hq_th = 0, hq_bits = 0;  // kernel 2: the hit queue's slots per wave (0: none, the ray queue), H, and the bounce list's bits per entry
    int copy = kCopyFast;          // KernelCopy
    int tris = 0;                  // kernels 0 and 1: the instantiation with the mesh (TRIS)
    int typ = 0;                   // kernels 2 and 4: the instantiation for the usual analytic scene (TYP)
    int max32 = 0;                 // kernel 2: at most 32 spheres, one group of the sphere filter (MAX32)
    int uniform_a = 1;             // kernel 2: phase A shades a wave whose primaries all hit one shape from that shape's record as a scalar
                                   // (render_body.inc shade_primary_hits); FLUX_SPLIT_UNIFORM_A=0: the general step everywhere
    int cut_depth = kNoDepthCut;   // kernel 2: phase B ends a path whose hit at this depth would bounce (split_cut_depth): max_depth, or kNoDepthCut
    int tput = 0;                  // kernel 2: the take reads the context's throughput table (RenderParams::tput) -- the hit queue, and a
                                   // table laid out for this plan's hq_bits; 0: the kernel gets no table
    int axis = 0;                  // kernel 2, TYP: the first scan plane's axis (RenderParams::plane_axis, the AXIS instantiation); else 0
};
// The split kernel's depth cut for a launch of `p` with plan `L` (its hq_cap and hq_bits): the job's max_depth, or kNoDepthCut
int split_cut_depth(const RenderParams &p, const LaunchPlan &L);
LaunchPlan plan_render(const RenderParams &p, int variant, int math);
// The instantiation a render launch of `p` with plan `L` runs, as one word (flux_ctx_launch_plan's word 7: FLUX_PLAN_FLAG_* in
// include/flux_abi.h): the fields of `L` the launch copies into template and kernel arguments -- a function of the plan alone (`p`
// stays in the signature for its callers).  0 where there is nothing to launch.
uint32_t plan_flags(const RenderParams &p, const LaunchPlan &L);
// The kernel family a launch runs: the render kernels, or one of the per-pixel passes -- the feature buffers (aov_body.inc
// aov_kernel), the sample moments (moments_body.inc moments_kernel), one pass of the adaptive sampler over a work list
// (adaptive_body.inc adaptive_pass_kernel), the feature buffers at the first non-specular hit (aov_chain_body.inc aov_chain_kernel)
enum Pass { kPassRender = 0, kPassAov = 1, kPassMoments = 2, kPassAdaptive = 3, kPassAovChain = 4 };
// The same for any pass (kPassRender: plan_render).  Of a per-pixel pass `kernel` is 0 (or -1: nothing to do) and block, grid and
// LDS are what plan_render's STATIC branch computes -- render_static_kernel's two layouts and its per-lane stacks --, with
//   kPassAov       `copy` never kCopyFastDiel -- a first hit runs no lobe --, `lds` the per-lane BVH stack of a mesh scene and nothing
//                  else, `blocks` one wave per pixel in map_wave's order from 64 samples on;
//   kPassMoments   `copy` as kernel_copy answers: the kernel runs the lobes;
//   kPassAdaptive  the same, with `blocks` sized by the `entries` of the pass's work list instead of the pixel grid (-1: an empty list);
//   kPassAovChain  as kPassMoments: the kernel runs the delta lobes and, in STRICT, keeps their (f, s) stack.
// `variant` counts for kPassRender alone, `entries` for kPassAdaptive alone.
LaunchPlan plan_pass(Pass pass, const RenderParams &p, int variant, int math, uint64_t entries = 0);

// THE statement of which kernel instantiations render.hip compiles: whether `copy` holds the kernel of `pass` -- of kPassRender the
// one LaunchPlan::kernel names -- with these template arguments (STATS apart: every kernel that counts exists with and without).  An
// argument the kernel does not take must be 0.  The launcher asks it before it names an instantiation (render_body.inc
// launch_render_impl), and the CPU test asks it of every plan (plan_exists; tests/scene_build_selftest.cpp), so the planner cannot ask
// for a kernel that is not there.  A new template flag is a planner rule and a row here.
//   the per-pixel passes       <TRIS>: aov_kernel, moments_kernel, adaptive_pass_kernel, aov_chain_kernel in every copy, and so is
//                              shade_rays_kernel (flux_debug_shade, which has no plan).  That includes aov_kernel in the copy with the
//                              dielectric lobe: aov_chain_kernel ends a chain with its file's first_hit_fields, and the file comes whole;
//                              plan_pass never names that copy for kPassAov -- a first hit runs no lobe
//   0 static, 1 refill         <STATS, TRIS>: every copy
//   2 split                    <STATS, MAX32, TYP, HQ, AXIS>: FAST.  TYP (the usual analytic scene) only with MAX32, any HQ, any
//                              AXIS (the first scan plane's stored normal lies on that axis); without TYP, AXIS 0, any MAX32 and HQ.
//                              The copy with the dielectric lobe has neither TYP nor HQ (the hit queue)
//   3 BVH, binary tree         <STATS>: FAST
//   4 BVH, 4-wide tree         <STATS, LDS_SCENE, TYP>: FAST.  TYP only with LDS_SCENE, and not in the copy with the dielectric lobe
constexpr bool kernel_exists(int copy, int pass, int kernel, int tris, int typ, int max32, int hq, int axis, int lds_scene) {
    const bool flags_ok = (tris | typ | max32 | hq | lds_scene) >> 1 == 0 && axis >= 0 && axis <= 3;
    if (copy < kCopyStrict || copy > kCopyFastDiel || !flags_ok) return false;
    const bool fast = copy != kCopyStrict, diel = copy == kCopyFastDiel;
    const bool split_args = typ || max32 || hq || axis;  // (arguments of the split kernel alone; TYP: the 4-wide tree's too)
    if (pass != kPassRender) return pass > kPassRender && pass <= kPassAovChain && kernel == 0 && !split_args && !lds_scene;
    switch (kernel) {
        case 0:
        case 1: return !split_args && !lds_scene;
        case 2: return fast && !tris && !lds_scene && (typ ? max32 && !diel : axis == 0) && !(hq && diel);
        case 3: return fast && !tris && !split_args && !lds_scene;
        case 4: return fast && !tris && !max32 && !hq && !axis && (!typ || (lds_scene && !diel));
    }
    return false;
}
// ... asked of a plan: its fields as the launcher turns them into template arguments (true where there is nothing to launch)
constexpr bool plan_exists(Pass pass, const LaunchPlan &L) {
    return L.kernel < 0 || kernel_exists(L.copy, pass, L.kernel, L.tris, L.typ, L.max32, L.hq_cap > 0 ? 1 : 0, L.axis, L.lds_scene);
}

// LDS of the per-lane stacks of `lanes` lanes: the STRICT (f, s) recursion stack, 4 doubles per level, and the BVH traversal stack,
// one int per level
size_t lane_stacks_lds(int math, size_t depth, bool tris, size_t bvh_stack, size_t lanes);
// flux_debug_shade's kernel: its dynamic LDS (64-lane blocks)
size_t shade_rays_lds(const RenderParams &p, int math);

}  // namespace flux
