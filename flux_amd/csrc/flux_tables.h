// flux_tables.h -- host entry points of tables.hip / render.hip used by abi.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "flux_device.h"
#include "flux_plan.h"

namespace flux {

// MasterSampleSets::new (sampling.rs:13-33) for the sets of `sets` (slot m = global set first + m * stride; all S of
// them for {0, 1, S}) + shuffle_indices for all H rows and all S sets (sampling.rs:35-40), generated on the device.
// Synchronises `stream`.  phase_ms (optional) += {scratch allocation, launches + wait, scratch release} in ms.
hipError_t generate_tables(uint64_t seed, uint32_t S, SetRange sets, uint32_t D, uint32_t n, uint32_t H,
                           double2 *pix, double2 *disc, double *hemi, int32_t *rowperm, int32_t *invperm,
                           hipStream_t stream, double *phase_ms = nullptr);
// The split kernel's sample order (flux_sample_order.h) of `sets` held sets: order[slot][k] = the k-th sample index phase A traces, from
// depth row 0 of the slot's hemi rows alone -- so a set's row is the same in whichever context holds it.  Sorted on the device
// (a stable segmented radix sort of (key, index) pairs: a permutation of 0 .. n n - 1 by construction), then dealt.  identity:
// order[slot][k] = k (FLUX_SAMPLE_ORDER=0).  Synchronises `stream`; phase_ms as generate_tables.
hipError_t generate_sample_order(uint32_t sets, uint32_t D, uint32_t n, const double *hemi, uint32_t *order, bool identity,
                                 hipStream_t stream, double *phase_ms = nullptr);
// pix_o[t] = pix[set's row][order[t]], disc_o likewise, for the `count` = sets * N held samples (DevSetRows::pix_o, disc_o).  Synchronises `stream`.
hipError_t generate_order_copies(size_t count, uint32_t N, const uint32_t *order, const double2 *pix, const double2 *disc, double2 *pix_o,
                                 double2 *disc_o, hipStream_t stream);
// One set of a samplers-crate generator (0 regular, 1 jittered, 2 multi-jittered, 3 correlated MJ) and,
// if d_hemi != nullptr, its to_hemisphere(.., 0.0) image [N][3].  Synchronises `stream`.
hipError_t generate_sampler_grid(int kind, uint64_t seed, uint32_t n, double *d_xy, double *d_hemi,
                                 hipStream_t stream);
// FAST glossy lobe factors of the pixel samples: gloss[s][i] = (cos 2 pi x, sin 2 pi x, log2(1 - y), 0) with
// flux_math.h's functions (render.hip, FAST arithmetic).  Asynchronous on `stream`.
hipError_t generate_gloss_table(const double2 *pix, size_t count, double *gloss, hipStream_t stream);
// The glossy lobe's angles for the scene's n <= kGlossExpSlots exponents: out[t][k] = (cos theta, sin theta) of sample t (of `count`
// held samples, `gloss` as generate_gloss_table wrote it) for inv_e1[k], `pad` >= n entries per sample (render.hip: bit for bit the
// values fast_bounce computes in the loop).  Asynchronous on `stream`.
hipError_t generate_glossx_table(const double *gloss, size_t count, const double *inv_e1, int n, int pad, double2 *out, hipStream_t stream);
// The lobe frames of the scene's n_rec hit records (RenderParams::lobe_frame; `frec` on the device): out[k] = {b1, b2} of record k, zeros
// for a sphere (render.hip: bit for bit the frame fast_bounce builds in the loop for a Matte hit of the record).  Asynchronous on `stream`.
hipError_t generate_lobe_frame_table(const DevHitRec *frec, int n_rec, double *out, hipStream_t stream);
// The corner-normal records (RenderParams::tri_attrs) of ONE mesh, by the slot -> triangle map the device already holds (DevTri::id):
// every slot s < n_tris whose triangle k = tris[s].id - first_id lies in [0, count) gets table[s] = stage[k] (nine doubles of
// [count][3][3], bytes 0..71 of the 128-B record) and DevTri::smooth = 1 -- or, with stage == nullptr, smooth = 0 and, where
// `table` is not null, zeros in those bytes.  Other slots, and the record's other bytes, are not touched.  Asynchronous on `stream`.
hipError_t gather_tri_normals(DevTri *tris, int n_tris, int first_id, int count, const double *stage, double *table, hipStream_t stream);
// The same for the corner colours of ONE mesh (flux_ctx_set_mesh_colors): nine f32 of [count][3][3] into bytes 72..107 of the record
// and DevTri::colored; the normals' bytes and DevTri::smooth are not touched.
hipError_t gather_tri_colors(DevTri *tris, int n_tris, int first_id, int count, const float *stage, double *table, hipStream_t stream);
hipError_t hemi_to_aos(size_t SD, size_t N, const double *in, double *out, hipStream_t stream);

// The rows p names by the kernels of `pass` (flux_plan.h; not kPassAdaptive): Camera::render (trace.rs:53-97) for kPassRender --
// variant: FLUX_KERNEL_*, which counts for it alone --, the first-hit feature buffers (aov_body.inc, p.out =
// [num_rows][W][FLUX_AOV_CHANNELS]) or the per-pixel sample moments (moments_body.inc, p.out = [num_rows][W][FLUX_MOMENT_CHANNELS]).
// math: FLUX_MATH_FAST / FLUX_MATH_STRICT (render_body.inc).  Runs what plan_pass answers for the same arguments.
hipError_t launch_pass(Pass pass, const RenderParams &p, int variant, int math, hipStream_t stream);

// One pass of the adaptive sampler over the work list `a` names (adaptive_body.inc), for the rows p names: N more samples of every
// listed pixel added to a.sums, a.passes counted up.  Runs what plan_pass (flux_plan.h) answers for kPassAdaptive and a.count entries.
hipError_t launch_adaptive(const RenderParams &p, const AdaptiveWork &a, int math, hipStream_t stream);
// the feature buffers at the first non-specular hit (aov_chain_body.inc), chains of at most `max_chain` >= 1 segments
hipError_t launch_aov_chain(const RenderParams &p, int max_chain, int math, hipStream_t stream);

// What the adaptive sampler runs between and after its passes (adaptive.hip; no lobe code).  `pixels` = rows * width of the call.
struct AdaptiveRule {
    double tau2, lum_floor;  // threshold squared, the floor of the mean luminance
    uint32_t nsamp, dilate;  // N, the Chebyshev radius of the dilation
};
// hot[p] per pixel from the state (sums [pixels][kAdaptiveSums], passes [pixels]), then the pixels within `dilate` of a hot one
// compacted into list, their number in *count (zeroed here first).  Two launches and one 4-byte memset, asynchronous on `stream`.
hipError_t launch_adaptive_select(const AdaptiveRule &rule, uint32_t rows, uint32_t width, const double *sums, const uint32_t *passes,
                                  unsigned char *hot, uint32_t *list, uint32_t *count, hipStream_t stream);
// The state as the moments layout ([pixels][FLUX_MOMENT_CHANNELS], n = N c in place of N) and the pass map.  Asynchronous on `stream`.
hipError_t launch_adaptive_finish(uint32_t nsamp, uint64_t pixels, const double *sums, const uint32_t *passes, double *out_moments,
                                  uint32_t *out_passes, hipStream_t stream);
// *reached (zeroed here first) = the pixels with passes[p] == max_passes.  Asynchronous on `stream`.
hipError_t launch_adaptive_count(uint32_t max_passes, uint64_t pixels, const uint32_t *passes, uint32_t *reached, hipStream_t stream);

// Scene::shade for caller-supplied rays (device pointers; rays = n x (origin, direction)).
hipError_t launch_shade_rays(const RenderParams &p, int math, const double *d_rays, int n, int depth, uint32_t set,
                             uint32_t index, double *d_rgb, int *d_hit, double *d_t, hipStream_t stream);

// flux_math.h under test: out[i] = fn(a[i], b[i]) on the device (b may be null).
hipError_t launch_fastmath_probe(int fn, const double *a, const double *b, double *out, size_t n,
                                 hipStream_t stream);
// flux_plane_axis.h on the device (render.hip plane_div_probe_kernel): plane_div_unscaled, num / den, and the votes' word on den
hipError_t launch_plane_div_probe(const double *num, const double *den, double *unscaled, double *quotient, int32_t *admit, size_t n,
                                  hipStream_t stream);

}  // namespace flux
