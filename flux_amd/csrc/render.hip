// render.hip -- the per-pixel render loop on gfx950 (MI355X), FP64.
//
// Replaces Camera::render (fluxcore/src/trace.rs:53-97) and everything it
// calls: Camera::ray_direction (trace.rs:44-51), Scene::shade / Scene::hit
// (scene.rs:156-172), BoundingBox::hit / Sphere::hit / Plane::hit
// (shapes.rs:98-217), the three path_shade impls (materials.rs:18-72), the
// three BRDFs (brdf.rs:19-79), to_unit_hemi (samplers/src/lib.rs:133-142) and
// Color::max_to_one (color.rs:35-44).
//
// Mapping to the machine (not a translation of the reference's recursion):
//  * one lane = one camera path; one BLOCK owns one pixel: its 1..4 waves take contiguous slices of the
//    pixel's samples and each walks its slice 64 at a time, so pixel/lens table reads are contiguous
//    across the wave (16 B per lane);
//  * blocks are ordered by sample set and dealt to the 8 XCDs so that the tables of the set being worked on
//    stay in that XCD's L2 (render_body.inc map_wave);
//  * the scene (<= a few dozen shapes) is read with a wave-uniform index -> scalar loads, operands sit in
//    SGPRs; only the nearest hit's record is gathered per lane;
//  * the reference's recursion  L = (f1 (*) ((f2 (*) (...)) * s2)) * s1  is run iteratively -- STRICT pushes
//    (f, s = n.wi/pdf) on a per-lane LDS stack and folds it from the deepest bounce outward (the reference's
//    multiplication order), FAST multiplies a register throughput;
//  * SPLIT kernel (FAST, analytic scenes, the default from 256 spp): PRIMARY segments -- all lanes of a wave sample
//    one pixel, so their rays are coherent -- are traced 64 at a time against the pixel's own candidate spheres
//    (a wave-uniform mask, scalar operands, uniform control flow) and shaded together; the continuing paths go
//    through a 64-entry LDS queue to the SECONDARY loop, where a lane whose path ended pops the next queued path
//    (ballot + mbcnt prefix), so lanes stay busy although path lengths differ (1..D segments);
//  * REFILL kernel (STRICT; 64..255 spp): the same refill discipline with primaries and secondaries mixed in one loop;
//    STATIC kernel (< 64 spp): lane l traces samples l, l+64, ...;
//  * BVH kernels (FAST mesh scenes): persistent lanes with a per-lane traversal state machine -- over a 4-wide tree of 64-B
//    nodes (boxes on a 16-bit grid, planes built by v_perm_b32, tested through v_pk_fma_f32) with 128-B leaf records that
//    hold both halves of a quad (render_bvh4_kernel), or over the binary tree of 32-B nodes (render_bvh_kernel, fallback);
//  * per-lane partial sums are combined in lane order, wave totals in wave order (a fixed tree => the image is
//    bit-reproducible run to run and independent of how the frame is split), then * 1/n^2, max_to_one, and the
//    3 doubles are written once.  No atomics.
//
// The loop body (render_body.inc) is compiled three times: STRICT under `#pragma clang fp contract(off)` with the
// reference's operation order, FAST under contract(fast) with flux_math.h (see render_body.inc's header), and FAST again with the
// dielectric lobe.  Which copy, kernel and instantiation a call runs, with what block, grid and LDS, is the launch plan's decision
// (launch_plan.cpp plan_render, host code compiled once); the launchers below only map the plan to a kernel.  Which instantiations
// each copy holds is stated once: flux_plan.h kernel_exists.
#include <type_traits>

#include "flux_device.h"
#include "flux_plan.h"
#include "flux_tables.h"
#include "flux_math.h"
#include "flux_moments.h"
#include "../../include/flux_abi.h"

// Tunables: NUMBERS only (overridable with -D, scripts/sweep_variants.py).  Every either/or of rounds 1-5 -- 45 boolean FLUX_*
// switches with one shipped value and a measured verdict -- was folded into the code in round 6 (same ISA before and after,
// profiles/r06_experiments/prune_flags/); the experiments' patches and logs stay under profiles/r0*_experiments/.  What is left
// here, in flux_plan.h (FLUX_BLOCK_THREADS, FLUX_WPE_SPLIT, FLUX_HITQ_MIN_TAKE: the ones the launch planner reads too), in flux_device.h
// (FLUX_UNI_SPHERES, FLUX_BVH_WIDE_MAX_STACK, FLUX_MAX_WAVES_PER_PIXEL, FLUX_MIN_SAMPLES_PER_WAVE) and in bvh.cpp / flux_bvh.h
// (FLUX_BVH_BINS, FLUX_BVH_COLLAPSE_MODE, FLUX_BVH_LEAF), plus the six -DFLUX_DEBUG_* instrumentation hooks of render_body.inc (never
// in the product build), is the whole list.
#ifndef FLUX_WAVES_PER_EU
#define FLUX_WAVES_PER_EU 3
#endif
#ifndef FLUX_WPE_BVH
#define FLUX_WPE_BVH 4            // waves/SIMD of the binary-tree BVH kernel (the fallback): 4 waves, nothing spilled -- at 5 it spills 11 VGPRs
#endif
#ifndef FLUX_WPE_BVH4
#define FLUX_WPE_BVH4 5           // waves/SIMD of render_bvh4_kernel: 96 VGPRs, nothing spilled, since round 4's register diet (before: 122 at 4)
#endif
#ifndef FLUX_BVH4_EARLY_AT
#define FLUX_BVH4_EARLY_AT 48     // render_bvh4_kernel leaves its node loop for the shading step as soon as this many walks have ended
#endif
#ifndef FLUX_BVH_REFILL_AT
#define FLUX_BVH_REFILL_AT 40     // lanes that must be waiting for shading before the wave leaves traversal (swept 16..64 with the leaf vote)
#endif
// the early exit leaves the node loop when EARLY_AT walks have ended and expects the shading step to follow: with
// EARLY_AT < REFILL_AT the wave would re-enter the loop on the same counts and never advance
static_assert(FLUX_BVH4_EARLY_AT >= FLUX_BVH_REFILL_AT,
              "FLUX_BVH4_EARLY_AT must not be below FLUX_BVH_REFILL_AT (render_bvh4_kernel would livelock)");
#ifndef FLUX_BVH_LEAF_NUM
#define FLUX_BVH_LEAF_NUM 2       // binary-tree kernel: the inner-node loop is left once the lanes holding a leaf outweigh the descending ones,
#define FLUX_BVH_LEAF_DEN 3       //     n_leaf * NUM > n_inner * DEN (swept: 1:1 178.4, 2:3 175.9, 1:2 176.4, 1:3 179.7, 3:2 178.8 ms at 1024 spp)
#endif
#ifndef FLUX_STRICT_SCAN_UNROLL
#define FLUX_STRICT_SCAN_UNROLL 4  // STRICT shape scan: records fetched this many at a time (scalar loads issued together); demo2 @16384 spp 1035 -> 1026 ms
#endif
#ifndef FLUX_WAVES_PER_EU_FAST
#define FLUX_WAVES_PER_EU_FAST 5  // FAST render_refill_kernel without meshes: 94 VGPRs, nothing spilled
#endif
#ifndef FLUX_WAVES_PER_EU_FAST_WIDE
#define FLUX_WAVES_PER_EU_FAST_WIDE 4  // FAST render_static_kernel (12 VGPRs spilled under the 5-wave cap) and the mesh instantiations of
#endif                                 // render_refill_kernel (15 spilled): 4 waves/SIMD, nothing spilled (round 5; they shared the cap tuned
                                       // for the refill kernel in round 1)

// A run-time value as a compile-time constant: f(std::integral_constant<int, v>{}) for the v in [LO, LO + N) that `v` is, found by
// halving the range; a `v` outside it is an error.  How the launchers turn plan fields into template arguments.
namespace flux {
template <int N, int LO = 0, class F>
static hipError_t with_const(int v, F &&f) {
    if constexpr (N == 1) return v == LO ? f(std::integral_constant<int, LO>{}) : hipErrorInvalidValue;
    else return v < LO + N / 2 ? with_const<N / 2, LO>(v, f) : with_const<N - N / 2, LO + N / 2>(v, f);
}
}  // namespace flux

// The loop itself lives in render_body.inc and is compiled twice (see its header): the STRICT
// arithmetic (reference operation order, no contraction) and the FAST arithmetic (FMA + flux_math.h).
#define FLUX_FAST 0
#define FLUX_DIEL 1  // (STRICT: the dielectric branch sits behind RenderParams::has_diel, render_body.inc fast_bounce / shade_hit)
#define FLUX_WPE FLUX_WAVES_PER_EU
#define FLUX_WPE_WIDE FLUX_WAVES_PER_EU
#pragma clang fp contract(off)
namespace flux {
namespace strict {
#include "render_body.inc"
#include "aov_body.inc"
#include "moments_body.inc"
#include "adaptive_body.inc"
#include "aov_chain_body.inc"
}  // namespace strict
}  // namespace flux
#undef FLUX_FAST
#undef FLUX_DIEL
#undef FLUX_WPE
#undef FLUX_WPE_WIDE

#define FLUX_FAST 1
#define FLUX_WPE FLUX_WAVES_PER_EU_FAST
#define FLUX_WPE_WIDE FLUX_WAVES_PER_EU_FAST_WIDE
#pragma clang fp contract(fast)
#define FLUX_DIEL 0
namespace flux {
namespace fast {
#include "render_body.inc"
#include "aov_body.inc"
#include "moments_body.inc"
#include "adaptive_body.inc"
#include "aov_chain_body.inc"
}  // namespace fast
}  // namespace flux
#undef FLUX_DIEL
// ... and a third time for the scenes that have a Dielectric (RenderParams::has_diel): the same kernels with the
// dielectric lobe in fast_bounce.  The copy above, which every other scene runs, is compiled without it, so under contract(fast)
// the fusion decisions in its lobe code are the ones it made before the material existed.
#define FLUX_DIEL 1
namespace flux {
namespace fast_diel {
#include "render_body.inc"
#include "aov_body.inc"  // (for first_hit_fields, which aov_chain_body.inc ends a chain with: aov_kernel itself is never launched from this copy)
#include "moments_body.inc"
#include "adaptive_body.inc"
#include "aov_chain_body.inc"
}  // namespace fast_diel
}  // namespace flux
#undef FLUX_DIEL
// FAST glossy-lobe factors of every pixel sample (RenderParams::gloss), compiled with the FAST arithmetic
// so that the table holds bit for bit what to_unit_hemi would compute inline.
namespace flux {
__global__ void gloss_fill_kernel(const double2 *__restrict__ pix, size_t count, double *__restrict__ gloss) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const double2 p = pix[t];
    double s, c;
    fastmath::fsincos2pi(p.x, s, c);
    double *o = gloss + t * 4;
    o[0] = c;
    o[1] = s;
    o[2] = fastmath::flog2(1.0 - p.y);
    o[3] = 0.0;
}
hipError_t generate_gloss_table(const double2 *pix, size_t count, double *gloss, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    gloss_fill_kernel<<<dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream>>>(pix, count, gloss);
    return hipGetLastError();
}
}  // namespace flux
#undef FLUX_FAST
#undef FLUX_WPE
#undef FLUX_WPE_WIDE
#pragma clang fp contract(off)

namespace flux {

// The glossy lobe's angles of every held sample for the scene's exponents (RenderParams::glossx): entry (t, k) of `pad` >= n per sample =
// (cos theta, sin theta) of to_unit_hemi for inv_e1[k], from the tabulated log2(1 - y) (gloss[t].z).  The operations are the ones
// fast_bounce performs per bounce where the table is absent, in its order and with its roundings -- the product rounded on its own,
// 2^x by fexp2_tab over kExp2Poly (RenderParams::exp2c holds the same values), 1 - c c as ONE fused multiply-add, fsqrt --, written
// out and compiled without contraction, so that a stored value is bit for bit the one the loop would compute.  Entries k >= n are zero.
struct GlossExps {
    double inv_e1[kGlossExpSlots];
};
__global__ void glossx_fill_kernel(const double *__restrict__ gloss, size_t count, GlossExps e, int n, int pad, double2 *__restrict__ out) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count * (size_t)pad) return;
    const size_t t = j / (size_t)pad;
    const int k = (int)(j - t * (size_t)pad);
    double2 v = make_double2(0.0, 0.0);
    if (k < n) {
        const double m_inv_e1 = k == 0 ? e.inv_e1[0] : k == 1 ? e.inv_e1[1] : k == 2 ? e.inv_e1[2] : e.inv_e1[3];
        const double cos_theta = fastmath::fexp2_tab(m_inv_e1 * gloss[t * 4 + 2], fastmath::kExp2Poly);
        const double sin_theta = fastmath::fsqrt(fastmath::ffma(-cos_theta, cos_theta, 1.0));
        v = make_double2(cos_theta, sin_theta);
    }
    out[j] = v;
}
hipError_t generate_glossx_table(const double *gloss, size_t count, const double *inv_e1, int n, int pad, double2 *out, hipStream_t stream) {
    if (count == 0 || n < 1 || n > kGlossExpSlots || pad < n) return count == 0 ? hipSuccess : hipErrorInvalidValue;
    GlossExps e{};
    for (int k = 0; k < n; k++) e.inv_e1[k] = inv_e1[k];
    const size_t threads = count * (size_t)pad;
    glossx_fill_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream>>>(gloss, count, e, n, pad, out);
    return hipGetLastError();
}

// The lobe frames of the hit records (RenderParams::lobe_frame): entry k = {b1, b2} of fast_bounce's frame around w = n for record k's
// stored normal and its own (ax, az); zeros for a sphere, whose normal depends on the hit.  The operations are the ones the FAST loop
// performs per Matte bounce, in the order and with the fusions its compiled code has (contract(fast) decides them there; here they are
// written out and compiled without contraction): a x n with one product rounded on its own in y and none in x and z (the 1 of
// a = (ax, 1, az) needs no product), |.|^2 summed as y y, + x x, + z z, frsqrt from the hardware's seed -- which is why the host cannot
// build the table --, the three scalings, and b1 x n with each first product rounded and the second fused.
__global__ void lobe_frame_fill_kernel(const DevHitRec *__restrict__ frec, int n_rec, double *__restrict__ out) {
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= n_rec) return;
    const DevHitRec R = frec[k];
    double b1x = 0.0, b1y = 0.0, b1z = 0.0, b2x = 0.0, b2y = 0.0, b2z = 0.0;
    if (R.shape_kind != kShapeSphere) {
        const double nx = R.cx, ny = R.cy, nz = R.cz, ax = R.ax, az = R.az;
        const double x = fastmath::ffma(-az, ny, nz);
        const double y = fastmath::ffma(az, nx, -(ax * nz));
        const double z = fastmath::ffma(ax, ny, -nx);
        const double dd = fastmath::ffma(z, z, fastmath::ffma(x, x, y * y));
        const double s = fastmath::frsqrt(dd);
        b1x = x * s;
        b1y = y * s;
        b1z = z * s;
        b2x = fastmath::ffma(nz, b1y, -(ny * b1z));
        b2y = fastmath::ffma(nx, b1z, -(nz * b1x));
        b2z = fastmath::ffma(ny, b1x, -(nx * b1y));
    }
    double *o = out + (size_t)k * 6;
    o[0] = b1x; o[1] = b1y; o[2] = b1z;
    o[3] = b2x; o[4] = b2y; o[5] = b2z;
}
hipError_t generate_lobe_frame_table(const DevHitRec *frec, int n_rec, double *out, hipStream_t stream) {
    if (n_rec <= 0) return hipSuccess;
    lobe_frame_fill_kernel<<<dim3((unsigned)((n_rec + 63) / 64)), dim3(64), 0, stream>>>(frec, n_rec, out);
    return hipGetLastError();
}

// One attribute of one mesh, gathered into leaf order (flux_tables.h gather_tri_normals, gather_tri_colors): one thread per DevTri
// slot.  V = double: the nine corner-normal components at byte 0 of the slot's record and DevTri::smooth; V = float: the nine
// corner-colour components at byte 72 and DevTri::colored.  The other attribute's bytes and flag are left alone.
template <class V>
__global__ void gather_tri_attribute_kernel(DevTri *__restrict__ tris, int n_tris, int first_id, int count, const V *__restrict__ stage,
                                            double *__restrict__ table) {
    constexpr bool kColors = sizeof(V) == sizeof(float);
    const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (s >= n_tris) return;
    const int k = tris[s].id - first_id;
    if (k < 0 || k >= count) return;
    if (table) {
        V *o = reinterpret_cast<V *>(table + (size_t)s * kTriAttrDoubles) + (kColors ? kTriColorFloat0 : 0);
        for (int j = 0; j < 9; j++) o[j] = stage ? stage[(size_t)k * 9 + j] : (V)0;
    }
    if (kColors) tris[s].colored = stage ? 1 : 0;
    else tris[s].smooth = stage ? 1 : 0;
}
template <class V>
static hipError_t gather_tri_attribute(DevTri *tris, int n_tris, int first_id, int count, const V *stage, double *table, hipStream_t stream) {
    if (n_tris <= 0 || count <= 0) return hipSuccess;
    if (stage && !table) return hipErrorInvalidValue;
    gather_tri_attribute_kernel<V><<<dim3((unsigned)((n_tris + 255) / 256)), dim3(256), 0, stream>>>(tris, n_tris, first_id, count, stage, table);
    return hipGetLastError();
}
hipError_t gather_tri_normals(DevTri *tris, int n_tris, int first_id, int count, const double *stage, double *table, hipStream_t stream) {
    return gather_tri_attribute<double>(tris, n_tris, first_id, count, stage, table, stream);
}
hipError_t gather_tri_colors(DevTri *tris, int n_tris, int first_id, int count, const float *stage, double *table, hipStream_t stream) {
    return gather_tri_attribute<float>(tris, n_tris, first_id, count, stage, table, stream);
}

// The launcher of the <TRIS> kernels -- the per-pixel passes and flux_debug_shade, which every copy compiles both ways
// (flux_plan.h kernel_exists): the plan's grid, block, LDS and TRIS, the copy's kernel pair, and what the kernel takes
template <class... A>
static hipError_t launch_tris_pair(const LaunchPlan &L, hipStream_t stream, void (*plain)(A...), void (*tris)(A...), const A &...args) {
    if (L.blocks > 0x7fffffffull) return hipErrorInvalidValue;
    const dim3 g((unsigned)L.blocks), b(L.block);
    (L.tris ? tris : plain)<<<g, b, L.lds, stream>>>(args...);
    return hipGetLastError();
}

// `call` with the names of the copy of the kernel bodies the plan names
#define FLUX_IN_COPY(L, call)                                             \
    switch ((L).copy) {                                                   \
        case kCopyStrict: { using namespace strict; return call; }        \
        case kCopyFast: { using namespace fast; return call; }            \
        case kCopyFastDiel: { using namespace fast_diel; return call; }   \
    }                                                                     \
    return hipErrorInvalidValue

// the kernel the launch planner names for the pass (launch_plan.cpp plan_pass), in the copy it names
hipError_t launch_pass(Pass pass, const RenderParams &p, int variant, int math, hipStream_t stream) {
    const LaunchPlan L = plan_pass(pass, p, variant, math);
    if (L.kernel < 0) return hipSuccess;
    switch (pass) {
        case kPassRender: FLUX_IN_COPY(L, launch_render_impl(L, p, stream));
        case kPassMoments: FLUX_IN_COPY(L, launch_tris_pair(L, stream, moments_kernel<false>, moments_kernel<true>, p));
        case kPassAov: FLUX_IN_COPY(L, launch_tris_pair(L, stream, aov_kernel<false>, aov_kernel<true>, p));
        case kPassAdaptive: break;  // (launch_adaptive: it needs the work list)
        case kPassAovChain: break;  // (launch_aov_chain: it needs the chain limit)
    }
    return hipErrorInvalidValue;
}

// one pass of the adaptive sampler, in the copy a render of the same job runs
hipError_t launch_adaptive(const RenderParams &p, const AdaptiveWork &a, int math, hipStream_t stream) {
    const LaunchPlan L = plan_pass(kPassAdaptive, p, 0, math, a.count);
    if (L.kernel < 0) return hipSuccess;
    FLUX_IN_COPY(L, launch_tris_pair(L, stream, adaptive_pass_kernel<false>, adaptive_pass_kernel<true>, p, a));
}

// the feature buffers at the first non-specular hit, chains of at most `max_chain` segments, in the copy a render of the same job runs
hipError_t launch_aov_chain(const RenderParams &p, int max_chain, int math, hipStream_t stream) {
    const LaunchPlan L = plan_pass(kPassAovChain, p, 0, math);
    if (L.kernel < 0) return hipSuccess;
    FLUX_IN_COPY(L, launch_tris_pair(L, stream, aov_chain_kernel<false>, aov_chain_kernel<true>, p, max_chain));
}

// flux_debug_shade has no planner entry: 64-lane blocks, one ray a lane, the per-lane stacks
hipError_t launch_shade_rays(const RenderParams &p, int math, const double *d_rays, int n, int depth, uint32_t set,
                             uint32_t index, double *d_rgb, int *d_hit, double *d_t, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    LaunchPlan L;
    L.copy = kernel_copy(p, math);
    L.blocks = ((uint64_t)n + 63) / 64;
    L.lds = shade_rays_lds(p, math);
    L.tris = p.n_tris > 0 ? 1 : 0;
    FLUX_IN_COPY(L, launch_tris_pair(L, stream, shade_rays_kernel<false>, shade_rays_kernel<true>, p, d_rays, n, depth, set, index, d_rgb,
                                     d_hit, d_t));
}
#undef FLUX_IN_COPY

// ---- flux_math.h under test: out[i] = fn(a[i], b[i]) computed on the device ----------------------
__global__ void fastmath_probe_kernel(int fn, const double *a, const double *b, double *out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = a[i], y = b ? b[i] : 0.0;
    double r = 0.0, s, c;
    switch (fn) {
        case 0: r = fastmath::frsqrt(x); break;
        case 1: r = fastmath::fsqrt(x); break;
        case 2: r = fastmath::fdiv(x, y); break;
        case 3: r = fastmath::flog2(x); break;
        case 4: r = fastmath::fexp2(x); break;
        case 5: r = fastmath::fpow_pos(x, y); break;
        case 6: fastmath::fsincos2pi(x, s, c); r = s; break;
        case 7: fastmath::fsincos2pi(x, s, c); r = c; break;
        case 8: r = __builtin_amdgcn_rsq(x); break;   // raw hardware seeds, for the record
        case 9: r = __builtin_amdgcn_rcp(x); break;
        default: break;
    }
    out[i] = r;
}

hipError_t launch_fastmath_probe(int fn, const double *a, const double *b, double *out, size_t n,
                                 hipStream_t stream) {
    if (n == 0) return hipSuccess;
    fastmath_probe_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(fn, a, b, out, n);
    return hipGetLastError();
}

// ---- flux_plane_axis.h under test: the reduced arms' unscaled division, IEEE `/` and the votes' word on den, on the device ----
// admit[i]: bit 0 the predicate as a function of the lane's den, bit 1 the lane's bit of the mask the split kernel's votes take
__global__ void plane_div_probe_kernel(const double *num, const double *den, double *unscaled, double *quotient, int32_t *admit, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = num[i], y = den[i];
    unscaled[i] = plane_div_unscaled(x, y);
    quotient[i] = x / y;
    const unsigned long long lanes = fast::plane_div_admits_lanes(y);
    admit[i] = (plane_div_admits(y) ? 1 : 0) | ((lanes >> (threadIdx.x & 63)) & 1ull ? 2 : 0);
}

hipError_t launch_plane_div_probe(const double *num, const double *den, double *unscaled, double *quotient, int32_t *admit, size_t n,
                                  hipStream_t stream) {
    if (n == 0) return hipSuccess;
    plane_div_probe_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(num, den, unscaled, quotient, admit, n);
    return hipGetLastError();
}

}  // namespace flux
