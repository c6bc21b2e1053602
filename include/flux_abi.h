/*
 * flux_abi.h -- C ABI of the MI355X (gfx950) render path for jtdaugherty/flux.
 *
 * This is the drop-in boundary for fluxcore's per-pixel render loop.  In the
 * reference the path sits behind exactly three calls made by the LocalWorker
 * job loop (fluxcore/src/workers.rs:46-60):
 *
 *     Scene::from_data(job.scene_data, job.config)        workers.rs:46
 *     Camera::new(..., num_sets = image_width, ...)       workers.rs:47-54
 *     camera.render(&scene, unit) -> WorkUnitResult       workers.rs:60
 *
 * A GPU worker (a third sibling of LocalWorker / NetworkWorker behind
 * `trait Worker`, fluxcore/src/manager.rs:232-236) binds the entry points
 * below instead; INTEGRATION.md shows the Rust `extern "C"` block.
 *
 * Plain pointers and sizes only; no C++/torch types.  All floating point is
 * IEEE f64 as in the reference.  Functions return 0 on success or a negative
 * FLUX_E_* code; flux_last_error() gives the message for the calling thread
 * (the reference panics instead -- workers.rs:78, job.rs:67-70 -- a C ABI
 * must not unwind).
 */
#ifndef FLUX_ABI_H
#define FLUX_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: flux_ctx_bvh_info writes FLUX_BVH_INFO_WORDS = 16 words (version 1 documented 8) and takes the caller's capacity;
 *    flux_ctx_launch_plan added.
 * 3: the multi-GPU frame (flux_multi_*, flux_render_frame_multi) and flux_ctx_create_timing added. */
#define FLUX_ABI_VERSION 3

/* error codes */
#define FLUX_OK 0
#define FLUX_E_INVALID (-1)  /* bad argument (null, out-of-range row, root<1, depth<1 ...) */
#define FLUX_E_DEVICE (-2)   /* HIP runtime error / no usable gfx950 device */
#define FLUX_E_NOMEM (-3)    /* device or host allocation failed */
#define FLUX_E_IO (-4)       /* file output failed */

/* ShapeData variants: fluxcore/src/scene.rs:71-74 */
#define FLUX_SHAPE_SPHERE 0
#define FLUX_SHAPE_PLANE 1
/* EXTENSION (absent in the reference; its TODO.md asks for a finite area light): a closed disk, see flux_shape.
 * Added without an ABI version bump: a library that predates it rejects kind 2 in flux_ctx_create with
 * FLUX_E_INVALID ("unknown kind"), which is how a client detects support. */
#define FLUX_SHAPE_DISK 2
/* EXTENSION (absent in the reference): an axis-aligned box, see flux_shape.  Added without an ABI version bump, as the
 * disk: a library that predates it rejects kind 3 in flux_ctx_create with FLUX_E_INVALID ("unknown kind"). */
#define FLUX_SHAPE_BOX 3

/* MaterialData variants: fluxcore/src/shapes.rs:42-47 */
#define FLUX_MAT_MATTE 0       /* MatteData            shapes.rs:52-56 */
#define FLUX_MAT_EMISSIVE 1    /* EmissiveData         shapes.rs:61-64 */
#define FLUX_MAT_REFLECTIVE 2  /* ReflectiveData       shapes.rs:69-72 */
#define FLUX_MAT_GLOSSY 3      /* GlossyReflectiveData shapes.rs:77-81 */
/* EXTENSION (absent in the reference): Fresnel-sampled glass, see flux_material.  Added without an ABI version
 * bump: a library that predates it rejects kind 4 in flux_ctx_create with FLUX_E_INVALID ("unknown material
 * kind"), which is how a client detects support. */
#define FLUX_MAT_DIELECTRIC 4

/* MaterialData (shapes.rs:42-81) flattened:
 *   Matte     : color = diffuse_color, ambient = ambient_color (parsed but
 *               unused by path_shade, materials.rs:18-34), k = diffuse_coefficient
 *   Emissive  : color, k = power
 *   Reflective: color = reflect_color, k = reflect_amount
 *   Glossy    : color = reflect_color, k = reflect_amount, exponent = reflect_exponent
 *   Dielectric (extension, FLUX_MAT_DIELECTRIC): color = transmit_color, k = refraction_index
 *               (finite and > 0, else flux_ctx_create returns FLUX_E_INVALID); ambient and exponent
 *               are ignored.  Allowed on every shape and mesh.  A hit with shading normal n (as for
 *               the other materials), n^ = n/|n|, d^ = d/|d|, c = -d^.n^: from outside (c > 0)
 *               eta = k, m = n^; else eta = 1/k, m = -n^, c = -c.  F = 1 if 1 - (1 - c^2)/eta^2 < 0
 *               (total internal reflection), else the unpolarised Fresnel reflectance.  With u the
 *               z of hemi_sets[set][depth-1][sample]: u <= F reflects, wi = d^ + 2c m, weight 1;
 *               otherwise wi = d^/eta + (c/eta - c_t) m, weight color.  No emission, no ambient
 *               term, no eta^2 radiance factor.  DESIGN.md section 5c. */
typedef struct flux_material {
    int32_t kind;
    int32_t reserved;
    double color[3];
    double ambient[3];
    double k;
    double exponent;
} flux_material;

/* ShapeData (scene.rs:71-74) = SphereData (shapes.rs:18-23) | PlaneData
 * (shapes.rs:33-37).  sphere: p = center, radius, invert.  plane: p = point,
 * n = normal (used as given: never normalised or flipped, shapes.rs:135-152).
 * disk (extension, FLUX_SHAPE_DISK): p = centre, n = normal, radius (`invert` ignored).
 * Plane::hit's t = ((p - o).n) / (d.n), a hit iff t > T_MIN and the hit point q
 * (the next segment's origin) has |q - p|^2 <= radius^2; a non-finite t is a miss.
 * Two-sided, normal as given (as the plane's); it emits towards -n only
 * (materials.rs:44).  radius must be finite and >= 0 (0: a degenerate disk),
 * else flux_ctx_create returns FLUX_E_INVALID.  Ties: YAML index, as every shape.
 * box (extension, FLUX_SHAPE_BOX): p = corner0, n = corner1, `invert` honoured, radius ignored.
 * Every corner component must be finite and corner0[k] < corner1[k] on each axis, else
 * flux_ctx_create returns FLUX_E_INVALID (before any device work).  BoundingBox::hit's slabs
 * (shapes.rs:99-131) as a shape: per axis k = x, y, z: a_k = 1/d_k and (tmin_k, tmax_k) =
 * ((c0_k - o_k) a_k, (c1_k - o_k) a_k) if a_k >= 0, else swapped; t0 = max(tmin_x, max(tmin_y,
 * tmin_z)), t1 = min(tmax_x, min(tmax_y, tmax_z)) with the reference's max(a,b) = a > b ? a : b
 * and min(a,b) = a < b ? a : b.  A ray parallel to a slab that starts ON one of its planes has
 * 0 * inf = NaN there: those forms drop a NaN of the x or y slab (the slab then bounds nothing)
 * and hand a NaN of the z slab through, which is a miss.  No hit unless t0 < t1; then t = t0 (the
 * entry) if t0 > T_MIN, else t = t1 (the exit) if t1 > T_MIN, else no hit.  The face is on the
 * first axis k (x, y, z) with tmin_k == t (entry) resp. tmax_k == t (exit); the normal is that
 * face's outward unit axis (entry: -e_k if a_k >= 0 else +e_k; exit: the opposite), negated
 * for `invert`, never flipped towards the ray.  So an Emissive box emits outwards, an inverted
 * one inwards (a room), and a Dielectric box is entered at c > 0.  Ties: YAML index.
 * DESIGN.md section 5d. */
typedef struct flux_shape {
    int32_t kind;
    int32_t invert;
    double p[3];
    double n[3];
    double radius;
    flux_material material;
} flux_shape;

/* EXTENSION (absent in the reference: scene.rs:71-74 has Sphere | Plane only, TODO.md lists a Quad):
 * an indexed triangle mesh.  Semantics chosen to follow the reference's conventions for Plane
 * (shapes.rs:135-152): two-sided, hit iff t > T_MIN, geometric normal normalize((v1-v0) x (v2-v0))
 * stored per triangle and never flipped towards the ray.  Intersection is Moeller-Trumbore in f64
 * (DESIGN.md "Triangles and the BVH").  Hit order for the nearest-hit tie rule: all `shapes` first
 * (YAML order), then the triangles of meshes[0], meshes[1], ... in index order. */
typedef struct flux_mesh {
    uint64_t num_vertices;
    const double *vertices;  /* [num_vertices][3] */
    uint64_t num_triangles;
    const uint32_t *indices; /* [num_triangles][3] vertex indices */
    flux_material material;
} flux_mesh;

/* SceneData (scene.rs:40-49) with CameraSettings (:14-18), CameraData
 * (:53-58) and OutputSettings (:62-66) inlined.  `shapes` keeps YAML order:
 * Scene::hit resolves distance ties to the lowest index (scene.rs:156-160,
 * common.rs:17-23). */
typedef struct flux_scene_desc {
    const char *scene_name;
    uint64_t image_width;
    uint64_t image_height;
    double pixel_size;
    double background[3];
    double eye[3];
    double look_at[3];
    double up[3];
    double zoom_factor;
    double view_plane_distance;
    double focal_distance;
    double lens_radius;
    uint64_t num_shapes;
    const flux_shape *shapes;
    uint64_t num_meshes;      /* extension; 0 for reference scenes */
    const flux_mesh *meshes;
} flux_scene_desc;

/* JobConfiguration: fluxcore/src/job.rs:49-53 */
typedef struct flux_job_cfg {
    uint64_t sample_root;
    uint64_t max_trace_depth;
    uint64_t rows_per_work_unit;
} flux_job_cfg;

/* WorkUnit: fluxcore/src/job.rs:40-44 (row_end inclusive; job_id is
 * scheduler bookkeeping and stays on the caller's side) */
typedef struct flux_work_unit {
    uint64_t row_start;
    uint64_t row_end;
} flux_work_unit;

typedef struct flux_ctx flux_ctx;

uint32_t flux_abi_version(void);
const char *flux_last_error(void);

/* Number of usable devices (0 when no GPU is visible; never fails). */
int flux_device_count(void);

/* Identity of the library's sources, fixed at build time (flux_amd/build.py): "lib:<16 hex> kernels:<16 hex>" -- hashes of all
 * sources + flags, and of the device-code sources alone (render.hip, render_body.inc, tables.hip and the headers they include).
 * A profile summary under profiles/ records the id of the binary it was taken from; bench.py compares. */
const char *flux_build_id(void);

/* Brings the HIP runtime up on `device` -- device context, the first copy, the first kernel launch of this library's code object,
 * a stream -- so that the first flux_ctx_create on it costs what every later one does (7 ms for demo2 at 16384 spp instead of 30-130).
 * The reference's counterpart is LocalWorker::new building its rayon pool when the worker is made (workers.rs:27-38), before any
 * job's timer runs (manager.rs:145).  Optional; idempotent; safe from any thread. */
int flux_device_warmup(int device);

/* Replaces Scene::from_data (scene.rs:128-154) + Camera::new (trace.rs:26-42)
 * incl. MasterSampleSets::new (sampling.rs:13-33): copies the scene, uploads
 * it to HBM and generates the S = image_width sample sets of pixel / lens-disc
 * / hemisphere tables ON THE DEVICE.  `seed` is an addition: the reference
 * seeds from OS entropy (samplers/src/lib.rs:27-33); see DESIGN.md "RNG
 * contract".  The caller keeps ownership of `scene`. */
int flux_ctx_create(const flux_scene_desc *scene, const flux_job_cfg *cfg, uint64_t seed,
                    int device, flux_ctx **out);

/* flux_ctx_create for ONE RANK of a set-sharded render (flux_render_sets_device with the same first_set / set_stride):
 * the sample tables are generated and held only for the sets first_set + m*set_stride this rank owns -- 1/set_stride
 * of MasterSampleSets::new's work and memory (sampling.rs:13-33).  A set's contents depend on (seed, set index) only,
 * so they equal the full context's.  flux_render_rows* and flux_debug_shade need every set and are rejected on such a
 * context; flux_ctx_copy_table returns the held sets in slot order.  first_set < set_stride. */
int flux_ctx_create_sets(const flux_scene_desc *scene, const flux_job_cfg *cfg, uint64_t seed, int device,
                         uint64_t first_set, uint64_t set_stride, flux_ctx **out);

/* Drops Scene + Camera (workers.rs:73-74). NULL is a no-op. */
void flux_ctx_destroy(flux_ctx *ctx);

/* Replaces Camera::render (trace.rs:53-97) for one WorkUnit.  Writes
 * (row_end-row_start+1) * image_width * 3 doubles, row-major RGB, already
 * averaged over sample_root^2 samples and max_to_one-clamped -- exactly what
 * WorkUnitResult.rows holds (manager.rs:24-28).  Synchronous: returns after
 * the device->host copy.  out_rgb is caller-owned host memory. */
int flux_render_rows(flux_ctx *ctx, uint64_t row_start, uint64_t row_end, double *out_rgb);

/* Same render, device-resident: rows first_row, first_row+row_stride, ...
 * (num_rows of them) are written to d_out_rgb (device pointer, num_rows *
 * image_width * 3 doubles) asynchronously on `hip_stream` (a hipStream_t, or
 * NULL for the default stream).  This is what the multi-GPU path uses so that
 * the framebuffer gather (RCCL) never leaves HBM.  row_stride >= 1. */
int flux_render_rows_device(flux_ctx *ctx, uint64_t first_row, uint64_t row_stride,
                            uint64_t num_rows, void *d_out_rgb, void *hip_stream);

/* The same render sharded along the OTHER axis of the work: sample sets instead of rows.  Every pixel of a row
 * uses a different sample set (trace.rs:64-69: `idx` is a permutation of 0..num_sets, num_sets = image_width,
 * workers.rs:50), so "the pixels whose set is first_set + m*set_stride, m < num_sets" is exactly one pixel per
 * row per set -- a 1/G share of the image for set_stride = G, with perfect load balance, and the share whose
 * sample tables stay cache-resident (DESIGN.md "set-grouped order").  Writes, for every image row r and m <
 * num_sets, 3 doubles at d_out_rgb[(r*num_sets + m)*3]; the pixel's column is the c with
 * flux_ctx_copy_row_perm(r)[c] == first_set + m*set_stride.  Asynchronous on `hip_stream` like
 * flux_render_rows_device.  Needs sample_root^2 >= 64 (refill kernel). */
int flux_render_sets_device(flux_ctx *ctx, uint64_t first_set, uint64_t set_stride, uint64_t num_sets,
                            void *d_out_rgb, void *hip_stream);

/* First-hit feature buffers (extension; FLUX_ABI_VERSION unchanged -- a client detects support by the symbol): what a denoiser,
 * a compositor or an edge-aware filter takes beside the beauty pass.  For pixel (row, col) of a context that holds every sample
 * set, with set = row_perm(row)[col] % S and N = sample_root^2, take for every i < N the primary ray the render kernels build for
 * (row, col, set, i) (trace.rs:71-80: pixel sample pixel_sets[set][i], lens sample disc_sets[set][i]) and its first hit by
 * Scene::hit under the context's arithmetic (flux_ctx_set_math, the routing to STRICT for non-unit plane normals included) and
 * traversal (flux_ctx_set_traversal): T_MIN, ties to the lowest YAML index, triangles after all shapes.  Per sample:
 *               hit                                                                   miss
 *   albedo (3)  a(material)                                                           background
 *   normal (3)  the shading normal exactly as the bounce would use it: sphere         0
 *               ((o - c) + t d) invert / radius; plane / disk as stored (never
 *               normalised or flipped); box face axis (negated for `invert`);
 *               triangle's stored unit normal
 *   t           the hit distance                                                      -
 *   covered     1                                                                     0
 * a(m): Matte diffuse_coefficient * diffuse_color; Reflective / Glossy reflect_amount * reflect_color; Dielectric transmit_color;
 * Emissive power * color if -n.d > 0 (materials.rs:44, the side it emits to), else 0.  Values are not clamped.
 * The pixel's FLUX_AOV_CHANNELS doubles: [0..2] the mean albedo over the N samples, [3..5] the mean normal over the N samples (a
 * miss contributes 0), [6] depth = the sum of t over the hitting samples / their number, 0 if none (a plane's +inf hit passes
 * through as inf), [7] coverage = hitting samples / N.  Per-lane partial sums are combined in a fixed order, so the buffers are
 * bit-reproducible run to run and independent of how rows are grouped into calls.  DESIGN.md section 5e. */
#define FLUX_AOV_CHANNELS 8
#define FLUX_AOV_ALBEDO 0
#define FLUX_AOV_NORMAL 3
#define FLUX_AOV_DEPTH 6
#define FLUX_AOV_COVERAGE 7
/* Rows [row_start, row_end] inclusive into caller-owned host memory: (row_end-row_start+1) * image_width * FLUX_AOV_CHANNELS
 * doubles, row-major.  Synchronous, argument checks as flux_render_rows.  The call stages through a device buffer of its own:
 * the scratch framebuffer of flux_render_rows is neither resized nor reused. */
int flux_render_aov_rows(flux_ctx *ctx, uint64_t row_start, uint64_t row_end, double *out);
/* Device-resident: rows first_row + k*row_stride, k < num_rows, to d_out (device pointer, num_rows * image_width *
 * FLUX_AOV_CHANNELS doubles), asynchronously on `hip_stream`.  Argument checks as flux_render_rows_device: row_stride >= 1,
 * num_rows == 0 is a no-op, and a context of flux_ctx_create_sets is refused with FLUX_E_INVALID (every row uses every set).
 * One kernel beside the render kernels, with no atomics and no effect on flux_ctx_stats; its launch is recorded between the
 * context's two events, so flux_ctx_last_kernel_ms reports it when it is the most recent launch. */
int flux_render_aov_rows_device(flux_ctx *ctx, uint64_t first_row, uint64_t row_stride, uint64_t num_rows,
                                void *d_out, void *hip_stream);

/* Feature buffers at the first NON-SPECULAR hit (extension; FLUX_ABI_VERSION unchanged -- a client detects support by the symbol):
 * the same FLUX_AOV_CHANNELS doubles per pixel, taken where a sample's chain of delta bounces ends, so that what a mirror or a pane
 * of glass shows has edges a denoiser can follow.  DESIGN.md section 5i; tests/aov_chain_spec.py states the rule in numpy.
 * The frame is that of the first-hit buffers above: a context that holds every sample set, pixel (row, col), set =
 * row_perm(row)[col] % S, N = sample_root^2, the context's arithmetic (the routing to STRICT for non-unit plane normals included)
 * and traversal.  max_chain sets the chain limit K: 0 means K = max_trace_depth, 1..max_trace_depth is K itself, a larger value is
 * FLUX_E_INVALID (the hemisphere table holds no u for a deeper segment, and the render never traces one).  Per sample i:
 *   1. the primary ray the render builds for (row, col, set, i); k = 1, tsum = 0;
 *   2. the nearest hit exactly as the render finds it: Scene::hit with T_MIN, ties to the lowest YAML index, triangles after all
 *      shapes, and in FAST the skip of the sphere a segment leaves outwards;
 *   3. a miss ends the chain uncovered: albedo fold(background), normal 0, no depth term;
 *   4. a hit on a Reflective or a Dielectric with k < K bounces, bit for bit as the render kernels bounce at that vertex -- the
 *      mirror direction with weight reflect_amount * reflect_color and scale (n.wi) / pdf as the render evaluates it; for a
 *      Dielectric u = hemi_sets[set][k-1][i].z and the Fresnel choice of FLUX_MAT_DIELECTRIC, weight 1 for a reflection and
 *      transmit_color for a transmission --, then tsum += t, k += 1, and step 2 again;
 *   5. any other hit ends the chain covered -- Matte, Glossy, Emissive, and a Reflective or Dielectric reached at k == K, whose own
 *      a(m) is used: albedo fold(a(m)) with a(m) as above and the emissive facing test taken with THIS segment's direction, the
 *      shading normal of this hit by the rule above (in world space, not unfolded through the mirror), depth term tsum + t.
 * fold(x) is the render's fold of the path's bounces applied to x in place of the end-of-path radiance: in STRICT (f * x) * s from
 * the deepest bounce outward, in FAST the front-to-back throughput product times x.  Nothing is clamped: a NaN scale at a grazing
 * mirror hit passes through, and so does a plane's +inf hit.  GlossyReflective is NOT followed: it is a sampled lobe of finite
 * width.  The pixel's doubles, their means and the fixed combination order are those of the first-hit buffers.
 * Three identities: max_chain = 1 gives flux_render_aov_rows bit for bit; so does every max_chain on a scene without Reflective
 * and Dielectric; and on a scene whose other materials are all Emissive, with max_chain = 0, the albedo of a pixel none of whose
 * samples ends on a delta material at k == K is the unclamped mean radiance of the frame (which is why it carries the throughput).
 * Host entry: rows [row_start, row_end] inclusive, (row_end-row_start+1) * image_width * FLUX_AOV_CHANNELS doubles, synchronous,
 * staged through a device buffer of its own.  Argument checks as flux_render_aov_rows, plus the max_chain range. */
int flux_render_aov_chain_rows(flux_ctx *ctx, uint64_t row_start, uint64_t row_end, uint32_t max_chain, double *out);
/* Device-resident, asynchronously on `hip_stream`; argument checks as flux_render_aov_rows_device, plus the max_chain range.  One
 * kernel beside the render kernels, with no atomics and no effect on flux_ctx_stats; its launch is recorded between the context's
 * two events.  A job whose STRICT stacks exceed the LDS of a block is refused as flux_render_moments_rows_device refuses it. */
int flux_render_aov_chain_rows_device(flux_ctx *ctx, uint64_t first_row, uint64_t row_stride, uint64_t num_rows, uint32_t max_chain,
                                      void *d_out, void *hip_stream);

/* A feature-guided a-trous denoiser for low-sample frames (extension; FLUX_ABI_VERSION unchanged -- a client detects support by
 * the symbol).  DESIGN.md section 5f; tests/denoise_spec.py states the same filter in numpy.
 * Inputs: rgb [H][W][3] as flux_render_rows returns it, aov [H][W][FLUX_AOV_CHANNELS] as flux_render_aov_rows returns it, of
 * which a = the albedo, n = the normal, z = the depth are used (the coverage is not).
 * Parameters (FLUX_DENOISE_PARAM_WORDS doubles, or NULL for the defaults): [0] levels L, an integer in 1..8, default 5;
 * [1] sigma_l 2.0; [2] sigma_n 0.35; [3] sigma_z 0.1; [4] sigma_a 0.1 -- each finite and > 0; [5..7] reserved, 0.
 * With |v|^2 = (v0^2 + v1^2) + v2^2 and lum(c) = (0.2126 r + 0.7152 g) + 0.0722 b:
 *   usable      a pixel whose rgb, a and n are finite in every component, whose lum(rgb) is finite and whose z is not NaN (+inf
 *               is a depth).  An unusable pixel is copied to the output bit for bit and contributes to no other pixel.
 *   G(p, q)     = ((|n_p - n_q|^2 / sigma_n^2) + e_z) + |a_p - a_q|^2 / sigma_a^2, where, both depths finite,
 *               d = (z_p - z_q) / ((|z_p| + |z_q|) + 1e-300) and e_z = d^2 / sigma_z^2; otherwise e_z = 0 if z_p == z_q, else +inf.
 *   taps        of a usable p at step s: q = p + s (i, j), i, j in -2..2, rows (j) outer and columns (i) inner; a tap off the
 *               image or on an unusable pixel is skipped.
 *   variance    once, on the input, taps at step 1, l = lum(rgb): w = exp2(-min(G(p, q), 1100)), s0 = sum w, m = sum w l_q / s0,
 *               then over the same taps var_p = sum w (l_q - m)^2 / s0 (two passes: s2 / s0 - m^2 cancels).
 *   level k     = 0..L-1, s = 2^k, reading the previous level's c and var of all pixels (never in place):
 *               sd = sigma_l sqrt(var_p) + 1e-8,  w = (h_j h_i) exp2(-min(G(p, q) + |lum(c_p) - lum(c_q)| / sd, 1100)) with
 *               h = [1/16, 1/4, 3/8, 1/4, 1/16],  c'_p = sum w c_q / sum w,  var'_p = sum w^2 var_q / (sum w)^2.
 *   output      max_to_one(c_L) (color.rs:35-44) for a usable pixel.
 * Division and sqrt are IEEE, nothing is fused, sums run in tap order and there are no atomics: the result is bit-reproducible.
 * The filter roughly quarters the error of a noisy 1-16 spp frame; it can LOSE on a frame that is already clean (section 5f). */
#define FLUX_DENOISE_PARAM_WORDS 8
/* Host pointers: rgb and out_rgb hold width * height * 3 doubles, aov width * height * FLUX_AOV_CHANNELS.  Synchronous, on
 * `device`, in device memory of its own.  Every argument check runs before any device call: FLUX_E_INVALID for a null pointer,
 * width or height 0, width * height > 2^26, or a parameter outside the ranges above. */
int flux_denoise(int device, uint64_t width, uint64_t height, const double *rgb, const double *aov,
                 const double *params, double *out_rgb);
/* Doubles of device scratch flux_denoise_device needs for an image of this size (0 for a size it refuses). */
uint64_t flux_denoise_work_doubles(uint64_t width, uint64_t height);
/* The same filter on device pointers of `device`, asynchronously on `hip_stream`: 2 + L kernel launches.  d_rgb and d_aov are only
 * read.  `params` is a host pointer, read before the call returns.  Checked as flux_denoise, and FLUX_E_INVALID as well for
 * work_doubles < flux_denoise_work_doubles(width, height) and for d_out_rgb equal to d_rgb or d_work. */
int flux_denoise_device(int device, uint64_t width, uint64_t height, void *d_rgb, void *d_aov, const double *params,
                        void *d_out_rgb, void *d_work, uint64_t work_doubles, void *hip_stream);

/* Per-pixel sample moments (extension; FLUX_ABI_VERSION unchanged -- a client detects support by the symbol): the frame together
 * with the measured variance of its samples, which a denoiser, an adaptive sampler or a convergence report reads.  DESIGN.md
 * section 5g; tests/moments_spec.py states the same in numpy.  For pixel (row, col) of a context that holds every sample set,
 * with N = sample_root^2 >= 4: the N samples the render kernels trace for it, each to its full depth under the context's
 * arithmetic and traversal, L_i the radiance of sample i and l_i = (0.2126 L_i.r + 0.7152 L_i.g) + 0.0722 L_i.b.  The five sums
 * of r, g, b, l and l^2 are formed per lane and combined in the fixed order flux_render_rows under FLUX_KERNEL_STATIC combines
 * its three: no atomics, bit-reproducible, independent of how rows are grouped into calls.  The pixel's FLUX_MOMENT_CHANNELS doubles:
 *   [0..2] FLUX_MOMENT_RGB   the frame: mean = sum c * (1 / N), then max_to_one (color.rs:35-44) -- bit for bit the pixel
 *                            flux_render_rows writes under FLUX_KERNEL_STATIC
 *   [3]    FLUX_MOMENT_VAR   the variance of the estimate lum(channels 0..2): (s2 / N) * k^2, with k = 1 / max(mean.r, mean.g,
 *                            mean.b) where that maximum exceeds 1 (the factor max_to_one applied), else 1
 *   [4..6] FLUX_MOMENT_MEAN  the mean radiance before max_to_one
 *   [7]    FLUX_MOMENT_S2    the sample variance of the luminance, s2 = max(0, sum l^2 - (sum l * sum l) / N) / (N - 1)
 * The max(0, .) keeps a NaN; nothing else is clamped, so a NaN or inf sample shows in channels 3 and 7.  The one-pass form of s2
 * carries a relative error of about N 2^-53 (1 + m^2 / s2), m the mean luminance: rounding level at preview sample counts. */
#define FLUX_MOMENT_CHANNELS 8
#define FLUX_MOMENT_RGB 0
#define FLUX_MOMENT_VAR 3
#define FLUX_MOMENT_MEAN 4
#define FLUX_MOMENT_S2 7
/* Rows [row_start, row_end] inclusive into caller-owned host memory: (row_end-row_start+1) * image_width * FLUX_MOMENT_CHANNELS
 * doubles, row-major.  Synchronous, argument checks as flux_render_aov_rows.  The call stages through a device buffer of its own:
 * neither the scratch framebuffer of flux_render_rows nor that of flux_render_aov_rows is resized or reused. */
int flux_render_moments_rows(flux_ctx *ctx, uint64_t row_start, uint64_t row_end, double *out);
/* Device-resident: rows first_row + k*row_stride, k < num_rows, to d_out (device pointer, num_rows * image_width *
 * FLUX_MOMENT_CHANNELS doubles), asynchronously on `hip_stream`.  Argument checks as flux_render_aov_rows_device, and
 * FLUX_E_INVALID as well for sample_root == 1: one sample has no variance (flux_denoise estimates one from the frame itself).  A
 * job whose per-lane stacks exceed the LDS limit is refused as flux_render_rows_device refuses it under FLUX_KERNEL_STATIC.  One
 * kernel beside the render kernels, with no effect on flux_ctx_stats; its launch is recorded between the context's two events. */
int flux_render_moments_rows_device(flux_ctx *ctx, uint64_t first_row, uint64_t row_stride, uint64_t num_rows,
                                    void *d_out, void *hip_stream);

/* flux_denoise with the MEASURED variance (tests/denoise_moments_spec.py): moments [H][W][FLUX_MOMENT_CHANNELS]
 * as flux_render_moments_rows returns it, of which rgb = channels 0..2 and v = channel 3 are used; aov, params (and their
 * defaults), levels, output, tap skipping and bit-reproducibility as flux_denoise.  It is that filter with exactly two changes:
 *   usable      a pixel must additionally have v finite and >= 0.
 *   variance    replaces the spatial estimate: over the same step-1 taps in the same order, with the same
 *               w = exp2(-min(G(p, q), 1100)):  var_p = sum w v_q / sum w, in one pass.
 * The prefilter matters: at 4 spp up to half of the pixels have all samples equal, and a variance of exactly 0 would make such
 * a pixel refuse every neighbour.  Argument checks as flux_denoise. */
int flux_denoise_moments(int device, uint64_t width, uint64_t height, const double *moments, const double *aov,
                         const double *params, double *out_rgb);
/* The same on device pointers of `device`, asynchronously on `hip_stream`: 2 + L kernel launches.  d_moments and d_aov are only
 * read.  flux_denoise_work_doubles is the scratch size for this call too.  Checked as flux_denoise_device (d_out_rgb may be neither
 * d_moments nor d_work). */
int flux_denoise_moments_device(int device, uint64_t width, uint64_t height, void *d_moments, void *d_aov, const double *params,
                                void *d_out_rgb, void *d_work, uint64_t work_doubles, void *hip_stream);

/* Smooth meshes (extension; FLUX_ABI_VERSION unchanged -- a client detects support by the symbol): three CORNER NORMALS per
 * triangle of a mesh, interpolated at the hit.  DESIGN.md section 5j; tests/smooth_spec.py states the same rule in numpy.
 * flux_mesh's layout is pinned, so the normals arrive through this call: corner_normals is a host pointer laid out
 * [num_triangles][3 corners][3], in the mesh's own triangle and corner order, and num_triangles must equal the mesh's count.
 * corner_normals == NULL with num_triangles == 0 clears the mesh back to facet normals.
 *   Checks, on the host at the time of the call and before any device call: every component finite, n.n finite and > 0.  Each
 *   normal is then normalised in f64, n / sqrt(n.n), IEEE.
 *   For a hit on triangle (v0, e1, e2) of such a mesh by the segment (o, d) the barycentrics are recomputed when the hit is
 *   shaded, with the hit test's own expressions:  p = d x e2,  inv = 1 / (e1.p),  s = o - v0,  u = (s.p) inv,  q = s x e1,
 *   v = (d.q) inv.  Then  w = (1 - u) - v,  m = (w n0 + u n1) + v n2 per component,  l2 = (m.x^2 + m.y^2) + m.z^2,  and the shading
 *   normal is m / sqrt(l2) if l2 >= 1e-24, otherwise the stored facet normal (opposed corner normals; a NaN).
 *   That vector stands wherever the stored normal is read: the bounce of every material, the Emissive facing test, the normal
 *   channel of both feature buffers (and so the guides of both denoisers), flux_debug_shade.  It is never flipped towards the ray.
 *   A triangle of a mesh without normals keeps its stored normal bit for bit, whatever the scene's other meshes have; the hit
 *   test, the BVH, ties and t are untouched.
 * The call is synchronous -- no render of the context may be in flight on a caller's stream --; a table set earlier for the mesh
 * is replaced; renders before and after are otherwise independent; a failed call leaves the context as it was.
 * FLUX_E_INVALID, with a message naming the mesh and the first offending triangle and
 * corner: a null context, mesh >= the scene's num_meshes, a wrong count, a non-finite or zero normal.  Works on the contexts of
 * flux_ctx_create and flux_ctx_create_sets and on the borrowed contexts of flux_multi_ctx: a flux_multi client sets the normals on
 * EVERY rank (a frame whose ranks disagree is not defined).  flux_ctx_device_bytes counts the table -- 128 B per triangle of the
 * scene, held while any mesh has normals. */
int flux_ctx_set_mesh_normals(flux_ctx *ctx, uint64_t mesh, const double *corner_normals, uint64_t num_triangles);

/* Vertex colours (extension; FLUX_ABI_VERSION unchanged -- a client detects support by the symbol): three CORNER COLOURS per
 * triangle of a mesh, interpolated at the hit and multiplied into the material's colour.  DESIGN.md section 5k;
 * tests/color_spec.py states the same rule in numpy.  corner_colors is a host pointer laid out [num_triangles][3 corners][3 rgb], in
 * the mesh's own triangle and corner order, and num_triangles must equal the mesh's count.  corner_colors == NULL with
 * num_triangles == 0 clears the mesh's colours.
 *   Host, when the call is made and before any device call: every component x must satisfy x >= 0 and x <= FLT_MAX (finite, and
 *   rounding to a finite f32; -0.0 is accepted; a NaN, a negative value, an infinity and anything larger are refused).  Each
 *   component is stored as (float)x, round-to-nearest-even: the stored corner colours k0, k1, k2.
 *   Device, where a hit on a triangle with colours is shaded: u, v are exactly the barycentrics of flux_ctx_set_mesh_normals --
 *   p = d x e2,  inv = 1 / (e1.p),  s = o - v0,  u = (s.p) inv,  q = s x e1,  v = (d.q) inv -- computed once when the triangle has
 *   both normals and colours.  Per channel, with k* widened to f64 (exact):  g1 = k1 - k0,  g2 = k2 - k0,
 *   c = (k0 + u g1) + v g2,  c = fmax(c, 0.0).  fmax is IEEE maxNum: a NaN gives 0, and so does a rounding residue below 0.
 *   The material then acts as if its colour were colour (*) c, for all five materials: Matte diffuse_color, Reflective and Glossy
 *   reflect_color, Dielectric transmit_color (the reflected branch's weight stays 1), Emissive color.  On the device this is one
 *   multiply of the triple read from the material record (and of the albedo triple of both feature buffers) by c, at the place
 *   where the triple is read.  STRICT performs exactly these operations; FAST may contract them and uses its fast division for
 *   inv, as for the normals.  Equal corner colours k give c = k exactly for finite u, v; all-ones colours give the uncoloured
 *   frame bit for bit.
 *   Everything else about the hit -- the test, the BVH, ties, t, the normal -- is untouched, and a triangle of a mesh without
 *   colours reads and computes what it did, also beside a mesh that has them.
 * The colours share the 128-B per-triangle record of the corner normals (nine f32 in bytes 72..107): the table exists while any mesh
 * has normals or colours, flux_ctx_device_bytes counts it once -- 128 B per triangle of the scene --, and clearing the last
 * attribute of the last mesh frees it.
 * The call is synchronous -- no render of the context may be in flight on a caller's stream --; colours set earlier for the mesh
 * are replaced; a failed call leaves the context as it was.  FLUX_E_INVALID, before any device call, with a message naming the
 * mesh and the first offending triangle, corner and channel: a null context, mesh >= the scene's num_meshes, a wrong count, a bad
 * component.  Works on the contexts of flux_ctx_create and flux_ctx_create_sets and on the borrowed contexts of flux_multi_ctx: a
 * flux_multi client sets the colours on EVERY rank.  The one-call flux_render_frame_multi has no place for them. */
int flux_ctx_set_mesh_colors(flux_ctx *ctx, uint64_t mesh, const double *corner_colors, uint64_t num_triangles);

/* Adaptive sampling (extension; FLUX_ABI_VERSION unchanged -- a client detects support by the symbol): further sample sets of
 * N = sample_root^2 samples for the pixels whose measured variance is still high, and only for those.  DESIGN.md section 5h;
 * tests/adaptive_spec.py states the same rule in numpy.  A call covers a list of h rows of W columns of a context that holds every
 * sample set; N >= 4, S = the number of sample sets (the image width).
 *   state    per pixel the five running sums of r, g, b, l and l^2 (l as for the sample moments) and a pass count c, all 0 at first.
 *   rounds   r = 0, 1, ... while r < max_passes.  In rounds r < min_passes every pixel is active.  Afterwards, per pixel,
 *              n = N c,  m = sum l / n,  s2 = max(0, sum l^2 - (sum l * sum l) / n) / (n - 1),
 *              e2 = (s2 / n) / max(m, lum_floor)^2
 *            -- the squared relative standard error of the pixel's luminance estimate --, and the pixel is HOT iff
 *            e2 > threshold^2: a NaN is never hot, an inf stays hot up to max_passes.  A pixel is ACTIVE iff a hot pixel lies within
 *            Chebyshev distance `dilate` of it, in the call's local row and column index, clipped at the call's edges (a pixel whose
 *            N samples happened to agree has variance 0 and says nothing about its own error: its neighbours speak for it).  The
 *            call stops at the first round with no active pixel.
 *   a pass   of an active pixel draws the N samples of sample set (set0 + c) mod S -- set0 the set the row's permutation gives the
 *            pixel, c the pixel's OWN count, not the round --, traces each as flux_render_moments_rows traces a sample, combines
 *            the five per-lane sums into one total as that call does, adds each total to the running sum with one addition, and
 *            sets c += 1.  max_passes <= S, so no pixel reads a set twice.
 *   output   [h][W][FLUX_MOMENT_CHANNELS] doubles in the layout of the sample moments with n = N c in place of N (the mean is
 *            sum * (1.0 / n)), and a [h][W] uint32_t map of c.  With max_passes == 1 the eight channels are bit for bit those of
 *            flux_render_moments_rows.  flux_denoise_moments filters the buffer as it filters the sample moments, with each pixel's
 *            own variance.
 * No atomics on a pixel's state, two runs are bit-equal, and apart from the rows a call covers -- and, for dilate > 0, which rows
 * are neighbours within it -- the result depends on nothing: with dilate == 0 not on how rows are grouped into calls. */
typedef struct flux_adaptive_params {
    double threshold;     /* tau: finite, >= 0 */
    double lum_floor;     /* finite, > 0 */
    uint32_t min_passes;  /* >= 1 */
    uint32_t max_passes;  /* min_passes <= max_passes <= S */
    uint32_t dilate;      /* 0, 1 or 2 */
    uint32_t reserved;    /* must be 0 */
} flux_adaptive_params;
/* Starting values, not tuned ones.  tests/test_adaptive.py holds a quality run at them (DESIGN.md section 5h has its table and what
 * it suggests): against a uniform frame of at least as many samples the adaptive frame is level on demo1 and worse on demo2,
 * where nearly every pixel runs into max_passes; a preview is better served by a threshold of 0.15 to 0.3. */
#define FLUX_ADAPTIVE_THRESHOLD 0.05
#define FLUX_ADAPTIVE_LUM_FLOOR 0.01
#define FLUX_ADAPTIVE_MIN_PASSES 1
#define FLUX_ADAPTIVE_MAX_PASSES 8
#define FLUX_ADAPTIVE_DILATE 1
/* info (optional, may be null): rounds run, pixel-passes traced (samples traced = N times that), pixels that reached max_passes, 0 */
#define FLUX_ADAPTIVE_INFO_WORDS 4
/* `params` points to a flux_adaptive_params, which the calls only read, and out_passes / d_out_passes to uint32_t; both are
 * declared void * because the header keeps to the pointer types its bindings already map.
 * Rows [row_start, row_end] inclusive into caller-owned host memory: out_moments (rows * image_width * FLUX_MOMENT_CHANNELS
 * doubles) and out_passes (rows * image_width uint32_t), row-major.  Synchronous.  FLUX_E_INVALID, before any device call and each
 * with a message of its own, for null params, a threshold that is not finite or negative, a lum_floor that is not finite or not
 * positive, min_passes < 1, max_passes < min_passes, dilate > 2 and a non-zero reserved word; then for a null context, a context
 * of flux_ctx_create_sets, sample_root == 1, max_passes > S, null outputs and rows outside the image. */
int flux_render_adaptive_rows(flux_ctx *ctx, uint64_t row_start, uint64_t row_end, void *params, double *out_moments,
                              void *out_passes, uint64_t info[FLUX_ADAPTIVE_INFO_WORDS]);
/* Device-resident: rows first_row + k*row_stride, k < num_rows (the call's local rows 0 .. num_rows - 1), to d_out_moments and
 * d_out_passes (device pointers) on `hip_stream`; num_rows == 0 is a no-op.  Checked as above, and row_stride >= 1.  NOT
 * asynchronous: after each selection the host reads the 4-byte count of active pixels back to size the next pass and to stop at 0
 * -- one synchronisation of `hip_stream` per round beyond min_passes --, and once more behind the last kernel where `info` is
 * given; without `info`, and with max_passes == min_passes, the call only enqueues.  State and work list live in buffers of the
 * context, grown on demand.  A job whose per-lane stacks exceed the LDS limit is refused as flux_render_moments_rows_device
 * refuses it.  No effect on flux_ctx_stats; flux_ctx_last_kernel_ms afterwards is the span from the call's first launch to its
 * last. */
int flux_render_adaptive_rows_device(flux_ctx *ctx, uint64_t first_row, uint64_t row_stride, uint64_t num_rows, void *params,
                                     void *d_out_moments, void *d_out_passes, uint64_t info[FLUX_ADAPTIVE_INFO_WORDS],
                                     void *hip_stream);

/* Render-kernel variants (all produce the same image within rounding):
 *   0 = default (FLUX_KERNEL_SPLIT where it applies, else FLUX_KERNEL_REFILL; STATIC below 64 spp)
 *   1 = FLUX_KERNEL_STATIC: one lane per sample, lanes idle once their path ends
 *   2 = FLUX_KERNEL_REFILL: persistent lanes refilled with the pixel's next
 *       sample by ballot/prefix compaction */
#define FLUX_KERNEL_DEFAULT 0
#define FLUX_KERNEL_STATIC 1
#define FLUX_KERNEL_REFILL 2
/*   3 = FLUX_KERNEL_SPLIT: FLUX_MATH_FAST, scenes without meshes and with <= 64 spheres, >= 64 spp: primary
 *       segments (coherent: all lanes of a wave sample one pixel) and secondary segments run in separate passes
 *       of the wave, joined by an LDS queue; elsewhere it behaves as FLUX_KERNEL_REFILL */
#define FLUX_KERNEL_SPLIT 3
int flux_ctx_set_kernel(flux_ctx *ctx, int variant);

/* Arithmetic of the render kernels -- both FP64 end to end, both checked against the oracle at the
 * north-star tolerance (1e-4 per channel):
 *   FLUX_MATH_FAST (default): the reference's estimator evaluated for the machine -- FMA contraction,
 *       division/sqrt/pow/sincos from flux_math.h (<= ~2 ulp), no BoundingBox::hit pre-test (the sphere quadratic
 *       implies its answer, except that a ray with direction.z == 0 whose origin lies on a z face of a sphere's box
 *       misses that sphere -- the box's 0 * inf = NaN, shapes.rs:121-130 -- which is reproduced by an explicit rule),
 *       path throughput multiplied front to back, bounce weights in closed form (glossy: cs ks, the Phong lobe cancels).
 *       That is the reference's value to rounding wherever surface normals are unit vectors.  A plane stored with a
 *       NON-unit normal makes reflected directions non-unit, lobes under- / overflow and the reference's recursion meet
 *       zeros and infinities in its own order (NaN pixels): a scene that has one is rendered with the STRICT arithmetic
 *       whatever this setting says, so the reference's NaN pixels appear exactly (flux_ctx_launch_plan reports the
 *       arithmetic in use).  WHAT THAT COSTS: STRICT renders demo2 at 16384 spp in 0.80 s where FAST
 *       takes 0.20 s, and a mesh scene also loses both traversal kernels -- so `normal: [0, 2, 0]`, or a normal typed to four
 *       digits ([0.7071, 0, 0.7071]: |n|^2 = 0.99997), is a 4 x slower scene than the same plane normalised to double
 *       precision.  The test is |n.n - 1| > 4 eps and is not looser on purpose: FAST takes every direction as a unit vector,
 *       and a normal that is off by 3e-5 bends every reflection off it by as much, which is above the parity tolerance.
 *       One exception: where the STRICT arithmetic cannot run the job at all (its LDS recursion stack holds 31 levels of
 *       max_trace_depth), such a scene stays with FAST and the reference's long-form glossy weights, as before round 4;
 *   FLUX_MATH_STRICT: the reference's operation order, no contraction, IEEE division/sqrt, OCML
 *       pow/sincos, BoundingBox::hit before every sphere, (f,s) stack folded deepest bounce first. */
#define FLUX_MATH_FAST 0
#define FLUX_MATH_STRICT 1
int flux_ctx_set_math(flux_ctx *ctx, int mode);

/* Triangle traversal (extension): 0 = BVH with a per-lane LDS stack (default), 1 = brute force over
 * all triangles in index order (the definition the BVH must reproduce exactly; parity tests). */
#define FLUX_TRAVERSE_BVH 0
#define FLUX_TRAVERSE_BRUTE 1
/* the BVH, but the FAST state-machine kernel walks the BINARY tree (32-B nodes, one record per triangle: round 2's kernel,
 * otherwise only the fallback for meshes whose 4-wide tree needs too deep a stack) -- a test hook that keeps it exercised */
#define FLUX_TRAVERSE_BVH_BINARY 2
int flux_ctx_set_traversal(flux_ctx *ctx, int mode);

/* Device time (ms, HIP events on the launch stream) of the most recent render
 * or feature-buffer kernel launched through this context; synchronises that launch. <0 on error. */
double flux_ctx_last_kernel_ms(flux_ctx *ctx);

/* Path statistics of the launches since the last reset (requires
 * flux_ctx_enable_stats(ctx,1) before rendering; off by default):
 * [0] samples, [1] ray segments, [2] Matte bounces, [3] glossy bounces,
 * [4] perfect-specular bounces, [5] emissive terminations, [6] misses,
 * [7] depth-exhausted paths, [8] BVH nodes visited, [9] triangles tested,
 * [10] dielectric reflections (total internal reflection included), [11] dielectric
 * transmissions (both 0 for a scene without FLUX_MAT_DIELECTRIC), [12..15] reserved (0).
 * Experiment builds with -DFLUX_DEBUG_TRIPS (never the product) write loop trip counts into
 * slots 10..15, over the dielectric counters. */
#define FLUX_NUM_STATS 16
int flux_ctx_enable_stats(flux_ctx *ctx, int on);
int flux_ctx_stats(flux_ctx *ctx, uint64_t out[FLUX_NUM_STATS], int reset);

/* BVH introspection (extension): out[0] nodes of the binary tree, [1] triangles, [2] its max depth, [3] max leaf size,
 * [4] its node bytes, [5] triangle-record bytes, [6] build microseconds; the 4-wide tree the FAST traversal kernel walks:
 * [7] nodes, [8] leaf records, [9] of them holding two triangles (the halves of a quad), [10] most stack entries at once
 * (one 32-bit entry per node with two children or more on a path: the 4-wide tree's depth), [11] node bytes, [12] leaf-record
 * bytes, [13] 1 if a full-frame render with the context's current settings walks the
 * 4-wide tree (flux_ctx_launch_plan's kernel == FLUX_PLAN_BVH4); [14..15] reserved (0).
 * Writes min(out_words, FLUX_BVH_INFO_WORDS) words: a caller states the capacity of its buffer. */
#define FLUX_BVH_INFO_WORDS 16
int flux_ctx_bvh_info(flux_ctx *ctx, uint64_t *out, uint64_t out_words);

/* What a render call WOULD launch with the context's current kernel variant, arithmetic and traversal -- the decision
 * itself (the library's one launch planner), not a restatement of it: for flux_render_rows* of `num_rows` rows when
 * num_sets == 0, for flux_render_sets_device of `num_sets` sets (all rows) otherwise.
 * out[0] kernel (FLUX_PLAN_*), [1] threads per block, [2] blocks, [3] dynamic LDS bytes per block,
 * [4] waves that share one pixel's samples (K: 1, 2 or 4 -- from the sample count, and in the STRICT arithmetic the LDS its
 * recursion stack leaves), [5] the arithmetic the launch runs with (FLUX_MATH_*: STRICT also under FLUX_MATH_FAST when the
 * scene has a plane with a non-unit normal, see flux_ctx_set_math), [6] FLUX_ROUTE_*: NONE; TO_STRICT = FLUX_MATH_FAST was
 * requested, the scene has a plane with a non-unit normal, the launch runs STRICT (several times slower); KEPT_FAST = the same
 * scene, but max_trace_depth (and the mesh's BVH depth) leave no room for STRICT's LDS recursion stack, so the job stays FAST
 * with the reference's long-form glossy weights -- its pixels can differ from the reference's NaN pixels in the rarest orderings
 * of an overflow and a zero.  The decision depends on the job alone, not on flux_ctx_set_traversal.
 * [7] FLUX_PLAN_FLAG_*: the instantiation of that kernel the launch runs (0 for FLUX_PLAN_NONE; the word was reserved, 0, before
 * the flags were added).  Which bits can be set depends on the kernel; the environment switches that take a choice away
 * (the table that opens flux_amd/csrc/flux_switches.h; DESIGN.md "Environment switches") clear its bit. */
#define FLUX_PLAN_FLAG_TYP 0x1u          /* SPLIT, BVH4: the instantiation for the usual analytic scene (TYP) */
#define FLUX_PLAN_FLAG_MAX32 0x2u        /* SPLIT: at most 32 spheres, one group of the sphere filter (MAX32) */
#define FLUX_PLAN_FLAG_HITQ 0x4u         /* SPLIT: the hit queue (clear: the ray queue) */
#define FLUX_PLAN_FLAG_TPUT_TABLE 0x8u   /* SPLIT with the hit queue: the take reads the context's throughput table (clear: it multiplies the list up) */
#define FLUX_PLAN_FLAG_DEPTH_CUT 0x10u   /* SPLIT: phase B ends a path whose hit at the depth limit would bounce */
#define FLUX_PLAN_FLAG_UNIFORM_A 0x20u   /* SPLIT: phase A shades a one-shape wave from scalar registers */
#define FLUX_PLAN_FLAG_LDS_SCENE 0x40u   /* BVH4: the analytic set's records and the materials in LDS */
#define FLUX_PLAN_FLAG_TRIS 0x80u        /* STATIC, REFILL: the instantiation with the mesh */
#define FLUX_PLAN_FLAG_AXIS_SHIFT 8      /* bits 8-9, SPLIT with TYP: the first plane's axis the launch instantiates, 0 none, 1 x, 2 y, 3 z */
#define FLUX_PLAN_FLAG_AXIS_MASK 0x300u
#define FLUX_PLAN_FLAG_HQ_BITS_SHIFT 10  /* bits 10-15, SPLIT with the hit queue: bits per entry of a parked hit's bounce list */
#define FLUX_PLAN_FLAG_HQ_BITS_MASK 0xfc00u
#define FLUX_PLAN_FLAG_COPY_SHIFT 16     /* bits 16-17, every kernel: the copy of the kernels, 0 STRICT, 1 FAST, 2 FAST with the dielectric lobe */
#define FLUX_PLAN_FLAG_COPY_MASK 0x30000u
#define FLUX_ROUTE_NONE 0
#define FLUX_ROUTE_TO_STRICT 1
#define FLUX_ROUTE_KEPT_FAST 2
#define FLUX_PLAN_NONE (-1)    /* nothing to launch */
#define FLUX_PLAN_STATIC 0     /* render_static_kernel */
#define FLUX_PLAN_REFILL 1     /* render_refill_kernel */
#define FLUX_PLAN_SPLIT 2      /* render_split_kernel */
#define FLUX_PLAN_BVH_BINARY 3 /* render_bvh_kernel */
#define FLUX_PLAN_BVH4 4       /* render_bvh4_kernel */
#define FLUX_PLAN_WORDS 8
int flux_ctx_launch_plan(flux_ctx *ctx, uint64_t num_rows, uint64_t num_sets, int64_t out[FLUX_PLAN_WORDS]);

/* Introspection used by the parity tests (device -> host copies).
 * which: 0 = pixel_sets [S][N][2], 1 = disc_sets [S][N][2],
 *        2 = hemi_sets  [S][D][N][3] (converted from the device SoA layout). */
#define FLUX_TABLE_PIXEL 0
#define FLUX_TABLE_DISC 1
#define FLUX_TABLE_HEMI 2
/* 3 = the split kernel's sample order [S][N]: the k-th sample index a pixel of the set traces, as doubles (a permutation of 0 .. N-1
 * per set; the identity under FLUX_SAMPLE_ORDER=0) */
#define FLUX_TABLE_ORDER 3
int flux_ctx_copy_table(flux_ctx *ctx, int which, double *out, uint64_t out_doubles);
int flux_ctx_copy_row_perm(flux_ctx *ctx, uint64_t row, int32_t *out, uint64_t out_len);
int flux_ctx_camera_basis(flux_ctx *ctx, double uvw[9]); /* CameraBasis::new scene.rs:28-35 */
/* bytes of HBM held by the context's tables + scene */
uint64_t flux_ctx_device_bytes(flux_ctx *ctx);

/* Where the wall time of the flux_ctx_create* call that made this context went, in milliseconds.  The reference's timer
 * (manager.rs:145 -> 170) spans exactly this work -- Scene::from_data + Camera::new incl. MasterSampleSets::new run
 * inside it (workers.rs:46-54) -- so it is reported beside the render time (bench.py `reference_equivalent_s`).
 * out[FLUX_CREATE_MS_*]: TOTAL = the whole call; HOST = validation, scene records, BVH build (host arithmetic);
 * RUNTIME = device selection + the HIP runtime's lazy per-device initialisation (zero in a process that has used the
 * device before); ALLOC = device allocation; UPLOAD = host -> device copies of the scene; TABLES = the sample-table
 * kernels (MasterSampleSets::new, sampling.rs:13-33) incl. the wait for them; FREE = release of the generator's
 * scratch; OTHER = events and the rest.  The parts sum to TOTAL. */
#define FLUX_CREATE_MS_TOTAL 0
#define FLUX_CREATE_MS_HOST 1
#define FLUX_CREATE_MS_RUNTIME 2
#define FLUX_CREATE_MS_ALLOC 3
#define FLUX_CREATE_MS_UPLOAD 4
#define FLUX_CREATE_MS_TABLES 5
#define FLUX_CREATE_MS_FREE 6
#define FLUX_CREATE_MS_OTHER 7
#define FLUX_CREATE_TIMING_WORDS 8
int flux_ctx_create_timing(flux_ctx *ctx, double out_ms[FLUX_CREATE_TIMING_WORDS]);

/* The samplers crate's four generators, evaluated on the device (what sampler-debug plots,
 * sampler-debug/src/main.rs:48-57): kind 0 grid_regular (samplers/src/lib.rs:184-191), 1 grid_jittered
 * (lib.rs:35-44), 2 grid_multi_jittered (lib.rs:64-73; equals hemi-stream set 0 depth 0 before the
 * hemisphere map), 3 grid_correlated_multi_jittered (lib.rs:75-90; equals pixel_sets[0]).  Writes
 * sample_root^2 (x,y) pairs to out_xy and, if out_hemi != NULL, to_hemisphere(.., 0.0) of them
 * (lib.rs:129-142) as sample_root^2 (x,y,z) triples.  Host pointers. */
#define FLUX_SAMPLER_REGULAR 0
#define FLUX_SAMPLER_JITTERED 1
#define FLUX_SAMPLER_MULTI_JITTERED 2
#define FLUX_SAMPLER_CORRELATED_MULTI_JITTERED 3
int flux_sampler_grid(int device, int kind, uint64_t sample_root, uint64_t seed, double *out_xy, double *out_hemi);

/* Test hook: Scene::shade (scene.rs:162-172) on the device for `n` caller-supplied rays (rays = n x {origin[3],
 * direction[3]}, host memory), each traced from `depth` (1 = a primary ray) with sample (set_index, sample_index) of
 * the context's tables and the context's arithmetic (flux_ctx_set_math).  out_rgb: n x 3 (un-clamped radiance, what
 * Scene::shade returns); out_hit: first hit per ray as the shape's YAML index, num_shapes + triangle index, or -1
 * (Scene::hit, scene.rs:156-160); out_t: its distance.  out_hit / out_t may be NULL. */
int flux_debug_shade(flux_ctx *ctx, uint64_t n, const double *rays, uint64_t depth, uint64_t set_index,
                     uint64_t sample_index, double *out_rgb, int32_t *out_hit, double *out_t);

/* Test hook for csrc/flux_math.h: out[i] = fn(a[i], b[i]) evaluated ON THE DEVICE (host pointers in,
 * host pointer out; b may be NULL for unary functions).  fn: 0 frsqrt, 1 fsqrt, 2 fdiv, 3 flog2,
 * 4 fexp2, 5 fpow_pos, 6 sin(2 pi a), 7 cos(2 pi a), 8 raw v_rsq_f64, 9 raw v_rcp_f64. */
int flux_debug_fastmath(int device, int fn, const double *a, const double *b, double *out, uint64_t n);

/* Test hook for csrc/flux_plane_axis.h: for n operand pairs (host pointers), evaluated ON THE DEVICE, out_unscaled[i] = the split
 * kernel's unscaled first-plane division of num[i] by den[i], out_quotient[i] = num[i] / den[i], out_admit[i] = what the kernel's votes
 * say of den[i]: bit 0 the predicate (plane_div_admits), bit 1 the lane's bit of the wave mask the votes take. */
int flux_debug_plane_div(int device, const double *num, const double *den, double *out_unscaled, double *out_quotient,
                         int32_t *out_admit, uint64_t n);

/* ---- one frame on the GPUs of one node ------------------------------------------------------------------------------
 * Replaces, for GPUs in ONE process, what RenderManager does with a job: the fan-out of the job to every worker
 * (fluxcore/src/manager.rs:156-162: one clone of the job per worker handle) and ImageBuilder's gather of their rows into
 * the image (manager.rs:316-324).  Here the fan-out is one context per device -- each holding ONLY its share of the
 * sample tables (flux_ctx_create_sets(g, G): 1/G of MasterSampleSets::new's work and memory) -- and the gather is ONE
 * collective, ncclAllGather (RCCL, over xGMI between the GPUs of a node) of the shares, after which the frame is
 * reassembled ON THE DEVICE by the row permutation and copied to the caller once.  The frame is bit-identical for every
 * number of devices and equal to flux_render_rows' (a pixel's value depends on (seed, row, column) only).
 *
 * How the frame is split (`shard`):
 *   FLUX_SHARD_SETS: rank g renders, in every row, the pixels whose sample set s has s mod G == g
 *       (flux_render_sets_device): one pixel per row per owned set, i.e. a 1/G share with the cost of an average pixel;
 *       needs sample_root^2 >= 64.  Measured 98 % of ideal at G = 8.
 *   FLUX_SHARD_ROWS: rank g renders rows g, g + G, ... (flux_render_rows_device with row_stride G) -- the reference's
 *       WorkUnit rows, interleaved; every rank then holds ALL sample tables.
 *   FLUX_SHARD_AUTO: sets where they apply, rows below 64 spp.
 *
 * RCCL is bound at run time (dlopen of librccl.so.1; an RCCL the process has already mapped -- PyTorch's -- is used as
 * it is), so the library has no link-time dependency on it; flux_multi_create fails with FLUX_E_DEVICE when none is
 * found.  The communicators of a device list are created once per process (ncclCommInitAll) and kept for later
 * flux_multi_create calls on the same list; flux_multi_release_comms() destroys them.
 * Threading: a flux_multi is used by one host thread at a time. */
#define FLUX_SHARD_AUTO 0
#define FLUX_SHARD_SETS 1
#define FLUX_SHARD_ROWS 2
/* Test hook, OR-ed into `shard`: the ranks may share devices (the same ordinal listed several times) and the all-gather is
 * replaced by device-to-device copies -- no RCCL is loaded or called.  Every other step (per-rank share contexts, launches,
 * padding, reassembly) is the product path, so G = 2, 3, 8 can be checked on a one-GPU box. */
#define FLUX_SHARD_LOOPBACK 0x100

typedef struct flux_multi flux_multi;

/* devices[0..num_devices): HIP device ordinals, all different; devices[0] assembles the frame.  The contexts are
 * created concurrently (one host thread per device) while the communicators come up. */
int flux_multi_create(const flux_scene_desc *scene, const flux_job_cfg *cfg, uint64_t seed, const int *devices,
                      uint64_t num_devices, int shard, flux_multi **out);
void flux_multi_destroy(flux_multi *m); /* NULL is a no-op */

/* Camera::render for the WHOLE image (every WorkUnit of Job::work_units at once) on all devices: writes
 * image_height * image_width * 3 doubles, row-major RGB, averaged and max_to_one-clamped (what ImageBuilder holds after
 * the last RowsReady, manager.rs:316-324).  Synchronous.  out_rgb is caller-owned host memory. */
int flux_multi_render_frame(flux_multi *m, double *out_rgb);
/* The same frame left in HBM: *d_frame_rgb points at image_height * image_width * 3 doubles on devices[0], valid until
 * the next render call on `m` or its destruction.  Synchronous (returns once every device has finished the gather). */
int flux_multi_render_frame_device(flux_multi *m, const void **d_frame_rgb);

/* flux_ctx_set_kernel / flux_ctx_set_math for every rank's context */
int flux_multi_set_kernel(flux_multi *m, int variant);
int flux_multi_set_math(flux_multi *m, int mode);
/* rank's context, borrowed (owned by `m`): for flux_ctx_launch_plan, statistics, tables */
int flux_multi_ctx(flux_multi *m, uint64_t rank, flux_ctx **ctx);

/* out[0] devices G, [1] the split in use (FLUX_SHARD_SETS / FLUX_SHARD_ROWS), [2] RCCL version code (ncclGetVersion),
 * [3] doubles each rank contributes to the all-gather (H * ceil(S / G) * 3 or ceil(H / G) * W * 3), [4] bytes of HBM held
 * by all ranks' contexts together, [5] bytes of the gather + frame buffers on all devices, [6] 1 if the communicators
 * were taken from the process-wide cache (an earlier flux_multi_create on the same device list), [7] reserved (0). */
#define FLUX_MULTI_INFO_WORDS 8
int flux_multi_info(flux_multi *m, uint64_t out[FLUX_MULTI_INFO_WORDS]);

/* Milliseconds.  [0] flux_multi_create wall time, [1] of it: the slowest rank's flux_ctx_create_sets, [2] of it:
 * communicator creation (0 when cached; runs beside the context creation), then of the most recent frame: [3] wall time of
 * the render call, [4] the slowest rank's render kernel (HIP events on its stream), [5] all-gather (events on devices[0]'s
 * stream: from its own kernel's end, so it includes the wait for slower ranks), [6] reassembly kernel, [7] device -> host
 * copy of the frame (0 for flux_multi_render_frame_device). */
#define FLUX_MULTI_TIMING_WORDS 8
int flux_multi_timing(flux_multi *m, double out_ms[FLUX_MULTI_TIMING_WORDS]);

/* Destroys the process-wide communicator cache (ncclCommDestroy); call when no flux_multi is alive.  Returns the number of
 * device lists released.  Never fails. */
int flux_multi_release_comms(void);

/* One call: flux_multi_create + flux_multi_render_frame + flux_multi_destroy (a job's whole life, manager.rs:145-170).
 * devices may be NULL: the first num_devices devices (num_devices == 0: all visible ones). */
int flux_render_frame_multi(const flux_scene_desc *scene, const flux_job_cfg *cfg, uint64_t seed, const int *devices,
                            uint64_t num_devices, int shard, double *out_rgb);

/* Job::work_units (job.rs:65-88), including its `i < H-1` loop guard.  Writes
 * at most `cap` units and returns the number the reference would issue, or a
 * negative code (rows_per_work_unit == 0 panics in the reference). */
int64_t flux_work_units(uint64_t image_height, uint64_t rows_per_work_unit, flux_work_unit *out,
                        uint64_t cap);

/* Image::write (image.rs:43-61): ASCII P3, maxval 65535, `(c*65535.99) as
 * u16`, one pixel per line; rows whose rows_present[r]==0 (never received) are
 * written as zeros.  rows_present may be NULL (all present). */
int flux_write_ppm(const char *path, const double *rgb, uint64_t width, uint64_t height,
                   const uint8_t *rows_present);

#ifdef __cplusplus
}
#endif
#endif /* FLUX_ABI_H */
