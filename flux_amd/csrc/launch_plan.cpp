// launch_plan.cpp -- the launch planner: which render kernel instantiation a call runs, with what block, grid and LDS (flux_plan.h).
// Plain host code, compiled once: render.hip launches what it answers, abi.hip checks its LDS against the limit and reports it
// (flux_ctx_launch_plan), and tests/scene_build_selftest.cpp pins its answers for the shipped scenes on the CPU.
#include <algorithm>

#include "flux_plan.h"
#include "flux_switches.h"
#include "../../include/flux_abi.h"

namespace flux {

KernelCopy kernel_copy(const RenderParams &p, int math) {
    if (math == FLUX_MATH_STRICT) return kCopyStrict;
    return p.has_diel ? kCopyFastDiel : kCopyFast;
}

size_t lane_stacks_lds(int math, size_t depth, bool tris, size_t bvh_stack, size_t lanes) {
    return (math == FLUX_MATH_STRICT ? depth * 4 * lanes * sizeof(double) : 0) + (tris ? bvh_stack * lanes * sizeof(int) : 0);
}

size_t shade_rays_lds(const RenderParams &p, int math) {
    return lane_stacks_lds(math, (size_t)p.max_depth, p.n_tris > 0, (size_t)p.bvh_stack, 64);
}

// The TYP instantiations: scan_shapes_fast's TYP turns these values into constants of the instantiation, and it leaves the disks'
// and the boxes' loops and the dielectric lobe out.  The split kernel's usual scene -- whose glossy bounces, if it has any, read the lobe's angles
// from the table (RenderParams::glossx: in TYP the arithmetic they replace is not compiled) ...
static bool split_typ(const RenderParams &p) {
    return p.n_sph <= 32 && p.glossy_long == 0 && p.unit_dirs == 1 && p.self_skip == 1 && p.env_short == 1 && p.n_uni == 1 &&
           p.fsph32 != nullptr && p.n_dsk == 0 && p.n_box == 0 && p.has_diel == 0 && (p.n_gloss_exp == 0 || p.gx_stride != 0);
}
// ... and the usual analytic set beside a mesh in render_bvh4_kernel, whose records it keeps in LDS (no environment shortcut there)
static bool bvh4_typ(const RenderParams &p, bool lds_scene) {
    return lds_scene && p.n_sph <= 32 && p.glossy_long == 0 && p.unit_dirs == 1 && p.self_skip == 1 && p.n_uni == 1 &&
           p.fsph32 != nullptr && p.n_dsk == 0 && p.n_box == 0 && p.has_diel == 0;
}

// K, the waves that share a pixel's samples in the refill and split kernels: the largest power of two
// <= min(N / FLUX_MIN_SAMPLES_PER_WAVE, FLUX_MAX_WAVES_PER_PIXEL), from the sample count only
static unsigned waves_per_pixel(uint32_t N) {
    unsigned K = 1;
    while (K * 2u <= (unsigned)FLUX_MAX_WAVES_PER_PIXEL && (uint64_t)K * 2u * FLUX_MIN_SAMPLES_PER_WAVE <= N) K *= 2u;
    return K;
}

// The split kernel's scene copy in LDS, and whether the kernel serves the scene at all (see plan_render)
static size_t split_scene_lds(const RenderParams &p) {
    return (size_t)hit_records(p) * sizeof(DevHitRec) + (size_t)p.n_sph * sizeof(DevScanSphere);
}
static bool split_serves(const RenderParams &p) { return p.n_tris == 0 && p.n_sph <= 64 && split_scene_lds(p) <= 16384; }

// Whether the split kernel at K waves per pixel runs this scene with the hit queue, and with what C, H and bits per list entry (the
// rule: plan_render's comment at its call)
static bool plan_hitq(const RenderParams &p, unsigned K, size_t scene_lds, uint32_t &cap, uint32_t &th, int &bits) {
    if (p.glossy_long != 0 || p.has_diel != 0) return false;
    const size_t granules = (size_t)128 * K / (4 * FLUX_WPE_SPLIT);
    const size_t per_wave = granules * 1280 > scene_lds + 96 ? (granules * 1280 - scene_lds - 96) / K : 0;
    cap = (uint32_t)(per_wave / kHitQBytesPerSlot) & ~1u;  // (even: the next wave's queue stays 8-byte aligned)
    cap = hitq_cap(cap);
    th = cap > 64u + FLUX_HITQ_MIN_TAKE ? std::min(64u, cap - 64u) : FLUX_HITQ_MIN_TAKE;
    th = hitq_take_at(th);
    bits = 1;
    while ((1 << bits) < hit_records(p)) ++bits;
    return cap >= 64u + th && bits * p.max_depth <= 32;
}

size_t tput_table_bytes(const RenderParams &p, int *bits_out) {
    uint32_t cap, th;
    int bits;
    // (a context cannot know which kernel its renders will ask for: the table is there for every job the split kernel would run with
    // the hit queue -- FAST arithmetic, 64 samples or more --, and a render that runs another kernel leaves it unread)
    if (p.nsamp < 64u || p.max_depth < 2 || !split_serves(p) || !plan_hitq(p, waves_per_pixel(p.nsamp), split_scene_lds(p), cap, th, bits))
        return 0;
    const int list_bits = bits * (p.max_depth - 1);  // (<= 32 - bits: plan_hitq)
    if (list_bits + 1 > 24) return 0;                // (the kernel forms the entry's byte offset with a 24-bit multiply)
    const size_t bytes = ((size_t)2 << list_bits) * kTputEntryBytes;
    if (bytes > kTputTableMaxBytes) return 0;
    if (bits_out) *bits_out = bits;
    return bytes;
}

// The depth cut.  A hit at depth max_depth that bounces has a child beyond the limit, which ends with L = 0 (scene.rs:164-165): the
// path adds 0 * throughput to its lane's sums and counts as depth_exhausted, and its last ray is never traced.  Phase B may end it
// where it classifies the hit.
//   The ray queue (no hit queue planned): phase B has run the bounce already, so the zero is folded with the very throughput the later
//   pass would fold it with -- a NaN product included -- and the bounce's counters are counted.  Admitted for every job; what goes is
//   the pass the lane would hold the dead path through.
//   The hit queue: the hit is not parked, so its take and its bounce go too, and the zero is folded with the throughput BEFORE that
//   bounce.  That is the same sum exactly when both throughputs are finite: +-0 added to a sum that started at +0.0 changes nothing,
//   0 * inf = NaN does.  So the launch needs the context's word that every such product is finite (RenderParams::tput_finite, judged
//   on the throughput table where the context builds it); a job that gets no table keeps parking.  The word is about the scene's
//   weights, not about the device's copy of the table: a context built with FLUX_THROUGHPUT_TABLE=0 multiplies the same products up
//   in the take and renders the same frame, bit for bit, as one with the table.  The statistics build counts the skipped bounce by the
//   record's material kind (no Dielectric: such a scene has no hit queue, plan_hitq).
// FLUX_SPLIT_DEPTH_CUT=0 (tests, A/B runs): no cut in either loop.
int split_cut_depth(const RenderParams &p, const LaunchPlan &L) {
    if (switch_off(kEnvSplitDepthCut)) return kNoDepthCut;
    if (L.hq_cap == 0) return p.max_depth;
    return p.tput_finite != 0 ? p.max_depth : kNoDepthCut;
}

// The waves of a launch in the grouped order (map_wave): 8 XCD slots x (floor(S/8) sets x rows + an eighth of the last S % 8 sets' rows)
static uint64_t grouped_waves(const RenderParams &p) {
    return 8ull * ((uint64_t)(p.set_count / 8) * (uint64_t)p.num_rows + ((uint64_t)(p.set_count % 8) * (uint64_t)p.num_rows + 7u) / 8u);
}

LaunchPlan plan_render(const RenderParams &p, int variant, int math) {
    LaunchPlan L;
    L.copy = kernel_copy(p, math);
    const bool fast = L.copy != kCopyStrict;
    const uint32_t N = p.nsamp;
    const uint64_t npix = (uint64_t)p.num_rows * (uint64_t)p.img_w;
    if (npix == 0 || p.set_count <= 0) return L;
    // default: SPLIT from 256 spp (below, a wave's slice is a few 64-sample batches and its drain dominates); SPLIT
    // itself falls back to REFILL where it does not apply (STRICT arithmetic, meshes, more than 64 spheres)
    if (variant == FLUX_KERNEL_DEFAULT) variant = N >= 256u ? FLUX_KERNEL_SPLIT : FLUX_KERNEL_REFILL;
    if (N < 64u) variant = FLUX_KERNEL_STATIC;  // nothing to refill from
    const uint32_t lpp = N >= 64u ? 64u : N;
    const uint32_t ppw = 64u / lpp;
    uint64_t waves = (npix + ppw - 1) / ppw;
    if (variant != FLUX_KERNEL_STATIC && p.num_sets == (uint32_t)p.img_w) waves = grouped_waves(p);
    // refill kernel: K waves per pixel (block = pixel), K from the sample count only
    unsigned K = variant != FLUX_KERNEL_STATIC ? waves_per_pixel(N) : 1u;
    const bool tris = p.n_tris > 0;
    // STRICT keeps 32 B of recursion stack per level and lane in LDS: fewer waves per pixel where four would not fit the
    // 64 KiB a block may have (K = 4 holds 7 levels, K = 1 31); still a function of the job alone, never of the sharding
    if (!fast && variant != FLUX_KERNEL_STATIC)
        while (K > 1u && lane_stacks_lds(math, (size_t)p.max_depth, tris, (size_t)p.bvh_stack, 64 * K) > 60 * 1024) K /= 2u;
    const unsigned block = (variant == FLUX_KERNEL_STATIC) ? FLUX_BLOCK_THREADS : 64u * K;
    const unsigned wpb = (variant == FLUX_KERNEL_STATIC) ? block / 64 : 1u;  // refill: `waves` counts pixel slots
    L.blocks = (waves + wpb - 1) / wpb;
    if (fast && variant != FLUX_KERNEL_STATIC && tris && p.bvh_stack > 0) {  // BVH scenes: the traversal state machine
        L.block = 64;  // one wave per pixel (its launch bounds): `blocks` already counts pixel slots
        // over the 4-wide tree (kernel 4; 32 stack entries = 8 KiB per wave still allow 5 waves/SIMD) unless its stack would
        // leave fewer than 3 waves/SIMD: then the binary tree's kernel (kernel 3)
        size_t lds4 = (size_t)(p.bvh4_stack > 0 ? p.bvh4_stack : 1) * 64 * sizeof(int);
        // the analytic set's records + the materials in LDS behind the stack (round 5) while they are small: a one-wave block must stay
        // within the 6 LDS granules (7 680 B) that 5 waves/SIMD leave it, and the copy is made once per pixel
        const size_t scene4 = (size_t)hit_records(p) * sizeof(DevHitRec) + (size_t)p.n_mats * sizeof(DevMaterial) +
                              (size_t)p.n_sph * sizeof(DevScanSphere);
        const bool lds_scene4 = lds4 + scene4 <= 7680;
        if (lds_scene4) lds4 += scene4;
        // ... and unless a path's bounces do not fit its 32-bit material list (render_bvh4_kernel: mat_bits per bounce)
        if (p.nodes4 != nullptr && p.bvh4_stack <= FLUX_BVH_WIDE_MAX_STACK) {
            L.kernel = 4;
            L.lds = lds4;
            L.lds_scene = lds_scene4 ? 1 : 0;
            L.typ = bvh4_typ(p, lds_scene4) ? 1 : 0;
        } else {
            L.kernel = 3;
            L.lds = (size_t)p.bvh_stack * 64 * sizeof(int);
        }
        return L;
    }
    // analytic scenes: primary / secondary passes.  The kernel keeps the scene's hit records and scan spheres in the block's LDS, so it
    // serves scenes whose records fit 16 KiB there (64 spheres -- the pixel mask's width -- leave room for 85 planes, demo2's 12 for 154;
    // until round 6 the rule was "at most 16 planes", and a seventeenth sent the scene to the refill kernel); larger analytic scenes
    // take the refill kernel, which reads the records from global memory (the launch plan says which)
    const size_t scene_lds = split_scene_lds(p);
    if (fast && variant == FLUX_KERNEL_SPLIT && split_serves(p)) {
        L.kernel = 2;
        L.block = block;
        L.waves_per_pixel = K;
        L.lds = (size_t)kQueueBytesPerWave * K + scene_lds;
        L.typ = split_typ(p) ? 1 : 0;
        L.max32 = p.n_sph <= 32 ? 1 : 0;
        // FLUX_SPLIT_UNIFORM_A=0 (tests, A/B runs): phase A's general shading step for every wave (render_body.inc shade_primary_hits)
        if (switch_off(kEnvSplitUniformA)) L.uniform_a = 0;
        // The hit queue: as many slots as the LDS leaves a wave at FLUX_WPE_SPLIT waves/SIMD -- the CU's 128 granules of
        // 1280 B shared by 4 * FLUX_WPE_SPLIT / K blocks, less the scene copy and the 96 B of `part` (demo2, K = 4: 25 granules, 7 568 B
        // a wave, 110 slots of 68 B; H = 46).  A scene that leaves fewer than 64 + H slots (H at least FLUX_HITQ_MIN_TAKE), or whose bounce list does not fit 32 bits or does
        // not give the throughput back exactly (long-form glossy weights: P.glossy_long), keeps the ray queue and the immediate bounce.
        // C depends on the scene only through the size of its records, so a disk in place of a plane changes no lane a sample runs in.
        // FLUX_SPLIT_HITQ_CAP / FLUX_SPLIT_HITQ_TAKE_AT override C (at most what fits) and H.
        // A scene with a dielectric keeps the ray queue too: a dielectric bounce's weight depends on the branch it took, which its hit
        // record does not tell.
        uint32_t cap, th;
        int bits;
        if (plan_hitq(p, K, scene_lds, cap, th, bits)) {
            L.hq_cap = (int)cap;
            L.hq_th = (int)th;
            L.hq_bits = bits;
            L.lds = (size_t)cap * kHitQBytesPerSlot * K + scene_lds;
        }
        L.cut_depth = split_cut_depth(p, L);
        // (the throughput product table only where it is laid out for this plan's list entries)
        L.tput = L.hq_cap > 0 && p.tput != nullptr && p.tput_bits == L.hq_bits ? 1 : 0;
        L.axis = L.typ ? p.plane_axis : 0;  // (the AXIS instantiations are TYP's)
        return L;
    }
    L.kernel = variant == FLUX_KERNEL_STATIC ? 0 : 1;
    L.block = block;
    L.waves_per_pixel = variant == FLUX_KERNEL_STATIC ? 1 : K;
    L.lds = lane_stacks_lds(math, (size_t)p.max_depth, tris, (size_t)p.bvh_stack, block);
    L.tris = tris ? 1 : 0;
    return L;
}

uint32_t plan_flags(const RenderParams &, const LaunchPlan &L) {
    if (L.kernel < 0) return 0;
    const bool split = L.kernel == 2;
    const bool hq = split && L.hq_cap > 0;
    uint32_t f = 0;
    if ((split || L.kernel == 4) && L.typ) f |= FLUX_PLAN_FLAG_TYP;
    if (split && L.max32) f |= FLUX_PLAN_FLAG_MAX32;
    if (hq) f |= FLUX_PLAN_FLAG_HITQ;
    if (L.tput) f |= FLUX_PLAN_FLAG_TPUT_TABLE;
    if (split && L.cut_depth != kNoDepthCut) f |= FLUX_PLAN_FLAG_DEPTH_CUT;
    if (split && L.uniform_a) f |= FLUX_PLAN_FLAG_UNIFORM_A;
    if (L.kernel == 4 && L.lds_scene) f |= FLUX_PLAN_FLAG_LDS_SCENE;
    if ((L.kernel == 0 || L.kernel == 1) && L.tris) f |= FLUX_PLAN_FLAG_TRIS;
    f |= ((uint32_t)L.axis << FLUX_PLAN_FLAG_AXIS_SHIFT) & FLUX_PLAN_FLAG_AXIS_MASK;
    if (hq) f |= ((uint32_t)L.hq_bits << FLUX_PLAN_FLAG_HQ_BITS_SHIFT) & FLUX_PLAN_FLAG_HQ_BITS_MASK;
    f |= ((uint32_t)L.copy << FLUX_PLAN_FLAG_COPY_SHIFT) & FLUX_PLAN_FLAG_COPY_MASK;
    return f;
}

// A per-pixel pass (aov_body.inc, moments_body.inc, adaptive_body.inc): `units` pixels or work-list entries in lane_group's layout
// (render_body.inc) -- 64 / N units per wave below 64 samples, one from there on, in the order given --, or the pixels in map_wave's
// order (`grouped`); FLUX_BLOCK_THREADS lanes a block, each with the (f, s) stack `stack_math` needs for `depth` levels and the BVH
// stack of a mesh scene.  `kernel` is 0, or -1 where there is nothing to do.
static LaunchPlan plan_pixel_pass(const RenderParams &p, KernelCopy copy, uint64_t units, int stack_math, size_t depth, bool grouped) {
    LaunchPlan L;
    L.copy = copy;
    const uint32_t N = p.nsamp;
    if (units == 0 || p.set_count <= 0 || N == 0) return L;
    const uint32_t ppw = N >= 64u ? 1u : 64u / N;
    const uint64_t waves = grouped ? grouped_waves(p) : (units + ppw - 1) / ppw;
    const unsigned wpb = FLUX_BLOCK_THREADS / 64;
    L.kernel = 0;
    L.block = FLUX_BLOCK_THREADS;
    L.blocks = (waves + wpb - 1) / wpb;
    L.tris = p.n_tris > 0 ? 1 : 0;
    L.lds = lane_stacks_lds(stack_math, depth, L.tris != 0, (size_t)p.bvh_stack, L.block);
    return L;
}

LaunchPlan plan_pass(Pass pass, const RenderParams &p, int variant, int math, uint64_t entries) {
    const uint64_t npix = (uint64_t)p.num_rows * (uint64_t)p.img_w;
    switch (pass) {
        case kPassRender: break;
        // the feature buffers: the refill kernels' pixel order from 64 samples on; a first hit runs no lobe (never the copy with the
        // dielectric one) and keeps no recursion stack whatever the arithmetic, so the BVH stack starts at the LDS base
        case kPassAov:
            return plan_pixel_pass(p, math == FLUX_MATH_STRICT ? kCopyStrict : kCopyFast, npix, FLUX_MATH_FAST, 0,
                                   p.nsamp >= 64u && p.num_sets == (uint32_t)p.img_w);
        // the sample moments: plan_render's STATIC branch at every sample count -- row-major pixels, the STRICT (f, s) stack and the
        // BVH stack per lane --, in the copy a render of the job runs
        // (the chain pass beside it: it runs the delta lobes of the same copy and keeps the same stacks)
        case kPassMoments:
        case kPassAovChain: return plan_pixel_pass(p, kernel_copy(p, math), npix, math, (size_t)p.max_depth, false);
        // one pass of the adaptive sampler: the same with the work list's entries in place of the pixel grid
        case kPassAdaptive: return plan_pixel_pass(p, kernel_copy(p, math), entries, math, (size_t)p.max_depth, false);
    }
    return plan_render(p, variant, math);
}

}  // namespace flux
