// denoise.hip -- flux_denoise*: the feature-guided a-trous filter of include/flux_abi.h (DESIGN.md sections 5f and 5g) over a frame of
// flux_render_rows, or the moments of flux_render_moments_rows, and the feature buffers of flux_render_aov_rows.
// tests/denoise_spec.py states the same filter in numpy.
//
// Its own translation unit under the build's default flags (-ffp-contract=off): every sum and product below keeps the order the
// header gives it, division and sqrt are IEEE, and the one function that differs from the numpy statement is fexp2 (flux_math.h).
//
// All kernels are one thread per pixel in blocks of 32 x 8 pixels (four 64-lane waves, each two image rows of 32 pixels):
//   denoise_pack_kernel       AoS input + aov -> planes of W*H doubles: albedo (3), normal (3), depth, colour (3).  An unusable pixel
//                             gets a NaN depth: no usable pixel has one, so the depth plane doubles as the usable flag.  <MOMENTS>: the
//                             input is the moments buffer ([H][W][8]: rgb = channels 0-2, v = channel 3), a pixel is usable only if v is
//                             finite and >= 0 as well, and v goes to the SECOND set's variance plane (14), which no launch reads before
//                             the first level has written it.
//   denoise_variance_kernel   flux_denoise: the guide-weighted variance of the luminance over 5 x 5, two passes over weights kept in
//                             registers.
//   denoise_varfilter_kernel  flux_denoise_moments: var_p = sum w v_q / sum w over the same taps and weights, one pass: plane 14 -> 10.
//   denoise_level_kernel      one a-trous level, launched `levels` times between two colour + variance plane sets (never in place);
//                             the last launch writes the AoS frame with max_to_one and copies the unusable pixels from the input.
//                             Steps 1-8 run as denoise_level_lds_kernel (one residue class of the step's lattice per block, staged
//                             in LDS), larger steps as plain global gathers: launch() has the measurement behind the choice.  The two
//                             differ in how a thread finds its pixel and where it reads a tap; level_pixel is the body of both.
// The luminance is recomputed from the colour wherever it is needed (three operations, the same bits as a stored plane).
// No atomics, a fixed tap order: bit-reproducible.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>

#include "../../include/flux_abi.h"
#include "flux_ctx.h"
#include "flux_math.h"
#include "flux_switches.h"

namespace flux {
namespace denoise {

constexpr int kTileW = 32, kTileH = 8;
constexpr int kPlanes = 15;  // albedo 0-2, normal 3-5, depth 6, colour A 7-9, variance A 10, colour B 11-13, variance B 14
constexpr int kHalo = 2;
constexpr uint64_t kMaxPixels = 1ull << 26;
constexpr double kEMax = 1100.0;   // exponents are clamped here: 2^-1100 is 0
constexpr double kSdFloor = 1e-8;
// the B3 spline's row [1/16, 1/4, 3/8, 1/4, 1/16]: products of two entries are exact
__device__ constexpr double kH5[5] = {0.0625, 0.25, 0.375, 0.25, 0.0625};

struct Frame {
    int32_t W, H, tiles_x;
    int32_t step;
    size_t npix;
    double *work;  // kPlanes planes of npix doubles
    double sigma_l, sn2, sz2, sa2;  // sigma_n^2, sigma_z^2, sigma_a^2: one rounding each, as the numpy statement
};

__device__ __forceinline__ double lum(double r, double g, double b) { return (0.2126 * r + 0.7152 * g) + 0.0722 * b; }
__device__ __forceinline__ double norm2(double x, double y, double z) { return (x * x + y * y) + z * z; }
__device__ __forceinline__ bool finite(double x) { return __builtin_fabs(x) < __builtin_inf(); }

// The guides of one pixel.
struct Guide {
    double a0, a1, a2, n0, n1, n2, z;
};
__device__ __forceinline__ Guide load_guide(const double *work, size_t npix, size_t idx, double z) {
    Guide g;
    g.a0 = work[0 * npix + idx];
    g.a1 = work[1 * npix + idx];
    g.a2 = work[2 * npix + idx];
    g.n0 = work[3 * npix + idx];
    g.n1 = work[4 * npix + idx];
    g.n2 = work[5 * npix + idx];
    g.z = z;
    return g;
}

// G(p, q) = ((|n_p - n_q|^2 / sigma_n^2) + e_z) + |a_p - a_q|^2 / sigma_a^2
__device__ __forceinline__ double guide_exponent(const Guide &p, const Guide &q, const Frame &f) {
    const double en = norm2(p.n0 - q.n0, p.n1 - q.n1, p.n2 - q.n2) / f.sn2;
    double ez;
    if (finite(p.z) && finite(q.z)) {
        const double d = (p.z - q.z) / ((__builtin_fabs(p.z) + __builtin_fabs(q.z)) + 1e-300);
        ez = (d * d) / f.sz2;
    } else {
        ez = p.z == q.z ? 0.0 : __builtin_inf();
    }
    const double ea = norm2(p.a0 - q.a0, p.a1 - q.a1, p.a2 - q.a2) / f.sa2;
    return (en + ez) + ea;
}

// This thread's pixel, or false past the image's edge.
__device__ __forceinline__ bool my_pixel(const Frame &f, int &x, int &y) {
    const int tile = blockIdx.x;
    x = (tile % f.tiles_x) * kTileW + (threadIdx.x & (kTileW - 1));
    y = (tile / f.tiles_x) * kTileH + (threadIdx.x >> 5);
    return x < f.W && y < f.H;
}

template <bool MOMENTS>
__global__ __launch_bounds__(kTileW *kTileH) void denoise_pack_kernel(Frame f, const double *__restrict__ in,
                                                                      const double *__restrict__ aov) {
    int x, y;
    if (!my_pixel(f, x, y)) return;
    const size_t idx = (size_t)y * f.W + x;
    const double *c = in + idx * (MOMENTS ? FLUX_MOMENT_CHANNELS : 3);
    const double *g = aov + idx * FLUX_AOV_CHANNELS;
    const double v = MOMENTS ? c[FLUX_MOMENT_VAR] : 0.0;
    bool ok = finite(c[0]) && finite(c[1]) && finite(c[2]) && finite(lum(c[0], c[1], c[2])) && finite(v) && v >= 0.0;
    for (int k = 0; k < 6; k++) ok = ok && finite(g[k]);
    const double z = g[FLUX_AOV_DEPTH];
    ok = ok && z == z;
    for (int k = 0; k < 6; k++) f.work[k * f.npix + idx] = g[k];
    f.work[6 * f.npix + idx] = ok ? z : __builtin_nan("");
    for (int k = 0; k < 3; k++) f.work[(7 + k) * f.npix + idx] = c[k];
    if (MOMENTS) f.work[14 * f.npix + idx] = v;
}

// The step-1 taps of this thread's pixel that the filter may use (on the image, usable), rows outer, columns inner: fn(q, t, w) for
// each, q the tap's pixel index, t = 0..24 its place in the window and w its weight from the guides alone.  Returns false, and calls
// nothing, for a thread without a pixel or with an unusable one (no tap ever reads that pixel's variance); else idx is the pixel.
template <class Fn> __device__ __forceinline__ bool guide_weighted_taps(const Frame &f, size_t &idx, Fn &&fn) {
    int x, y;
    if (!my_pixel(f, x, y)) return false;
    idx = (size_t)y * f.W + x;
    const double *work = f.work;
    const double zp = work[6 * f.npix + idx];
    if (zp != zp) return false;
    const Guide p = load_guide(work, f.npix, idx, zp);
#pragma unroll
    for (int j = -kHalo; j <= kHalo; j++) {
#pragma unroll
        for (int i = -kHalo; i <= kHalo; i++) {
            const int qx = x + i, qy = y + j;
            if (qx < 0 || qx >= f.W || qy < 0 || qy >= f.H) continue;
            const size_t q = (size_t)qy * f.W + qx;
            const double zq = work[6 * f.npix + q];
            if (zq != zq) continue;
            fn(q, (j + kHalo) * 5 + (i + kHalo), fastmath::fexp2(-__builtin_fmin(guide_exponent(p, load_guide(work, f.npix, q, zq), f), kEMax)));
        }
    }
    return true;
}

__global__ __launch_bounds__(kTileW *kTileH) void denoise_variance_kernel(Frame f) {
    const double *c0 = f.work + 7 * f.npix, *c1 = c0 + f.npix, *c2 = c1 + f.npix;
    double w[25], l[25];
#pragma unroll
    for (int t = 0; t < 25; t++) {
        w[t] = -1.0;  // a skipped tap
        l[t] = 0.0;
    }
    double s0 = 0.0, s1 = 0.0;
    size_t idx;
    if (!guide_weighted_taps(f, idx, [&](size_t q, int t, double wt) {
            w[t] = wt;
            l[t] = lum(c0[q], c1[q], c2[q]);
            s0 += w[t];
            s1 += w[t] * l[t];
        }))
        return;
    const double m = s1 / s0;
    double s2 = 0.0;
#pragma unroll
    for (int t = 0; t < 25; t++) {
        if (w[t] < 0.0) continue;
        const double d = l[t] - m;
        s2 += w[t] * (d * d);
    }
    f.work[10 * f.npix + idx] = s2 / s0;
}

__global__ __launch_bounds__(kTileW *kTileH) void denoise_varfilter_kernel(Frame f) {
    const double *v = f.work + 14 * f.npix;
    double s0 = 0.0, s1 = 0.0;
    size_t idx;
    if (!guide_weighted_taps(f, idx, [&](size_t q, int, double w) {
            s0 += w;
            s1 += w * v[q];
        }))
        return;
    f.work[10 * f.npix + idx] = s1 / s0;
}

// What a level sums over its taps.
struct Sums {
    double n0 = 0.0, n1 = 0.0, n2 = 0.0, den = 0.0, vnum = 0.0;
};
// One tap: hw = h_j h_i, (q0, q1, q2) and vq the tap's colour and variance, lp and sd the centre's luminance and sigma_l sqrt(var) + 1e-8.
__device__ __forceinline__ void add_tap(Sums &s, const Guide &p, const Guide &g, double lp, double sd, double hw, double q0, double q1,
                                        double q2, double vq, const Frame &f) {
    const double e = guide_exponent(p, g, f) + __builtin_fabs(lp - lum(q0, q1, q2)) / sd;
    const double wt = hw * fastmath::fexp2(-__builtin_fmin(e, kEMax));
    s.n0 += wt * q0;
    s.n1 += wt * q1;
    s.n2 += wt * q2;
    s.den += wt;
    s.vnum += (wt * wt) * vq;
}
// The level's result for pixel idx: into the planes `dst`, or, LAST, into the AoS frame with Color::max_to_one (color.rs:35-44).
template <bool LAST> __device__ __forceinline__ void store_pixel(const Sums &s, const Frame &f, size_t idx, int dst, double *out) {
    double r = s.n0 / s.den, g = s.n1 / s.den, b = s.n2 / s.den;
    if (LAST) {
        const double m1 = r > g ? r : g;
        const double m2 = m1 > b ? m1 : b;
        if (m2 > 1.0) {
            const double inv = 1.0 / m2;
            r *= inv;
            g *= inv;
            b *= inv;
        }
        out[idx * 3 + 0] = r;
        out[idx * 3 + 1] = g;
        out[idx * 3 + 2] = b;
    } else {
        double *d = f.work + (size_t)dst * f.npix;
        d[idx] = r;
        d[f.npix + idx] = g;
        d[2 * f.npix + idx] = b;
        d[3 * f.npix + idx] = s.vnum / (s.den * s.den);
    }
}

// One level for pixel idx.  `taps` says where a point of the pixel's 5 x 5 window is and reads it: Pos centre(); bool row(j) and
// bool at(j, i, pos) -- false for a row, and a point of a row, off the image --; depth(pos), guide(pos, z), and colour(pos, k), k = 0..2
// the source set's colour and 3 its variance.  (The row is asked once per j: with both tests in at() the last level by gathers takes
// 74 VGPRs instead of 70 and loses a wave per SIMD.)  Taps run rows outer, columns inner, as the header states the sum.  Only the LAST
// level touches `in`, the caller's input of in_stride doubles per pixel (3 for a frame, FLUX_MOMENT_CHANNELS for moments; rgb comes
// first in both), and `out`.
template <bool LAST, class Taps>
__device__ __forceinline__ void level_pixel(const Frame &f, const Taps &taps, size_t idx, int dst, const double *__restrict__ in,
                                            int in_stride, double *__restrict__ out) {
    const typename Taps::Pos c = taps.centre();
    const double zp = taps.depth(c);
    if (zp != zp) {  // unusable: bit for bit from the input, and nothing of it in the planes is ever read
        if (LAST)
            for (int k = 0; k < 3; k++) out[idx * 3 + k] = in[idx * in_stride + k];
        return;
    }
    const Guide p = taps.guide(c, zp);
    const double lp = lum(taps.colour(c, 0), taps.colour(c, 1), taps.colour(c, 2));
    const double sd = f.sigma_l * __builtin_sqrt(taps.colour(c, 3)) + kSdFloor;
    Sums s;
#pragma unroll
    for (int j = -kHalo; j <= kHalo; j++) {
        if (!taps.row(j)) continue;
#pragma unroll
        for (int i = -kHalo; i <= kHalo; i++) {
            typename Taps::Pos q;
            if (!taps.at(j, i, q)) continue;
            const double zq = taps.depth(q);
            if (zq != zq) continue;
            add_tap(s, p, taps.guide(q, zq), lp, sd, kH5[j + kHalo] * kH5[i + kHalo], taps.colour(q, 0), taps.colour(q, 1), taps.colour(q, 2),
                    taps.colour(q, 3), f);
        }
    }
    store_pixel<LAST>(s, f, idx, dst, out);
}

// Taps from the planes: the window of (x, y) is (x + i step, y + j step), and a position is a pixel index.
struct GlobalTaps {
    using Pos = size_t;
    const Frame &f;
    const double *src;  // the source set's colour and variance planes
    int x, y;
    __device__ Pos centre() const { return (size_t)y * f.W + x; }
    __device__ bool row(int j) const {
        const int qy = y + j * f.step;
        return qy >= 0 && qy < f.H;
    }
    __device__ bool at(int j, int i, Pos &q) const {
        const int qx = x + i * f.step;
        if (qx < 0 || qx >= f.W) return false;
        q = (size_t)(y + j * f.step) * f.W + qx;
        return true;
    }
    __device__ double depth(Pos q) const { return f.work[6 * f.npix + q]; }
    __device__ Guide guide(Pos q, double z) const { return load_guide(f.work, f.npix, q, z); }
    __device__ double colour(Pos q, int k) const { return src[k * f.npix + q]; }
};

// One level by global gathers: colour + variance planes `src` (7: set A, 11: set B) -> `dst`, or, LAST, the AoS frame `out`.  A block is
// a dense 32 x 8 tile of the image: every tap is one coalesced 256-B read per image row of the wave, served by the caches.
template <bool LAST>
__global__ __launch_bounds__(kTileW *kTileH) void denoise_level_kernel(Frame f, int src, int dst, const double *__restrict__ in,
                                                                       double *__restrict__ out, int in_stride) {
    int x, y;
    if (!my_pixel(f, x, y)) return;
    level_pixel<LAST>(f, GlobalTaps{f, f.work + (size_t)src * f.npix, x, y}, (size_t)y * f.W + x, dst, in, in_stride, out);
}

// The same level through LDS.  A step-s pass is s^2 independent dense 5 x 5 filters, one per residue class (x = alpha, y = beta mod s):
// a block takes 32 x 8 points of ONE class's lattice, stages them and their halo of 2 (36 x 12 points x 11 doubles = 38 016 B, one
// plane per quantity, so a wave's tap is two conflict-free runs of 32 consecutive doubles) and reads every tap from there.  Points off
// the image are staged with a NaN depth, the mark of a pixel no tap may use.  blockIdx.y = beta * s + alpha; blockIdx.x = the tile within
// the largest class's lattice (classes with a shorter lattice leave their last tiles empty).  Global reads and writes are s doubles apart.
constexpr int kLdsW = kTileW + 2 * kHalo, kLdsH = kTileH + 2 * kHalo, kLdsPoints = kLdsW * kLdsH, kLdsPlanes = 11;

// Taps from the tile (0-2 albedo, 3-5 normal, 6 depth, 7-9 colour, 10 variance): a position is a point of the tile, and every point
// of a window is there, so nothing is off the image.
struct LdsTaps {
    using Pos = int;
    const double (*tile)[kLdsPoints];
    int c;
    __device__ Pos centre() const { return c; }
    __device__ bool row(int) const { return true; }
    __device__ bool at(int j, int i, Pos &t) const {
        t = c + j * kLdsW + i;
        return true;
    }
    __device__ double depth(Pos t) const { return tile[6][t]; }
    __device__ Guide guide(Pos t, double z) const { return Guide{tile[0][t], tile[1][t], tile[2][t], tile[3][t], tile[4][t], tile[5][t], z}; }
    __device__ double colour(Pos t, int k) const { return tile[7 + k][t]; }
};

template <bool LAST>
__global__ __launch_bounds__(kTileW *kTileH) void denoise_level_lds_kernel(Frame f, int src, int dst, int lat_tiles_x,
                                                                           const double *__restrict__ in, double *__restrict__ out,
                                                                           int in_stride) {
    __shared__ double tile[kLdsPlanes][kLdsPoints];
    const int s = f.step;
    const int alpha = (int)blockIdx.y % s, beta = (int)blockIdx.y / s;
    const int u0 = ((int)blockIdx.x % lat_tiles_x) * kTileW, v0 = ((int)blockIdx.x / lat_tiles_x) * kTileH;  // the tile's first lattice point
    const double *work = f.work;
    for (int t = threadIdx.x; t < kLdsPoints; t += kTileW * kTileH) {
        const int u = u0 - kHalo + t % kLdsW, v = v0 - kHalo + t / kLdsW;
        const long qx = (long)alpha + (long)u * s, qy = (long)beta + (long)v * s;
        const bool on = u >= 0 && v >= 0 && qx < f.W && qy < f.H;
        const size_t q = on ? (size_t)qy * f.W + (size_t)qx : 0;
        const double zq = on ? work[6 * f.npix + q] : __builtin_nan("");
        tile[6][t] = zq;
        if (zq == zq) {
#pragma unroll
            for (int k = 0; k < 6; k++) tile[k][t] = work[k * f.npix + q];
#pragma unroll
            for (int k = 0; k < 4; k++) tile[7 + k][t] = work[(size_t)(src + k) * f.npix + q];
        }
    }
    __syncthreads();
    const int tx = threadIdx.x & (kTileW - 1), ty = threadIdx.x >> 5;
    const long x = (long)alpha + (long)(u0 + tx) * s, y = (long)beta + (long)(v0 + ty) * s;
    if (x >= f.W || y >= f.H) return;
    level_pixel<LAST>(f, LdsTaps{tile, (ty + kHalo) * kLdsW + tx + kHalo}, (size_t)y * f.W + (size_t)x, dst, in, in_stride, out);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------

static bool positive_finite(double x) { return std::isfinite(x) && x > 0.0; }

// params (or the defaults for nullptr) -> levels and f's sigmas; FLUX_E_INVALID for a value the header rules out
static int resolve_params(const double *params, int &levels, Frame &f) {
    double v[FLUX_DENOISE_PARAM_WORDS] = {5.0, 2.0, 0.35, 0.1, 0.1, 0.0, 0.0, 0.0};
    if (params)
        for (int k = 0; k < FLUX_DENOISE_PARAM_WORDS; k++) v[k] = params[k];
    if (!(v[0] >= 1.0 && v[0] <= 8.0) || v[0] != std::floor(v[0]))
        return fail(FLUX_E_INVALID, "flux_denoise: levels must be an integer in [1,8], got %g", v[0]);
    static const char *const names[] = {"sigma_l", "sigma_n", "sigma_z", "sigma_a"};
    for (int k = 0; k < 4; k++)
        if (!positive_finite(v[1 + k])) return fail(FLUX_E_INVALID, "flux_denoise: %s must be finite and > 0, got %g", names[k], v[1 + k]);
    for (int k = 5; k < FLUX_DENOISE_PARAM_WORDS; k++)
        if (!(v[k] == 0.0)) return fail(FLUX_E_INVALID, "flux_denoise: reserved parameter word %d must be 0, got %g", k, v[k]);
    levels = (int)v[0];
    f.sigma_l = v[1];
    f.sn2 = v[2] * v[2];
    f.sz2 = v[3] * v[3];
    f.sa2 = v[4] * v[4];
    return FLUX_OK;
}

static int check_size(uint64_t width, uint64_t height) {
    if (width == 0 || height == 0) return fail(FLUX_E_INVALID, "flux_denoise: image size %llux%llu: width and height must be >= 1",
                                               (unsigned long long)width, (unsigned long long)height);
    if (width > kMaxPixels || height > kMaxPixels || width * height > kMaxPixels)
        return fail(FLUX_E_INVALID, "flux_denoise: image size %llux%llu exceeds 2^26 pixels", (unsigned long long)width,
                    (unsigned long long)height);
    return FLUX_OK;
}

// How many of the first levels (steps 1, 2, 4, ...) run through LDS tiles instead of global gathers.  Measured on demo2 at 800 x 600
// (scripts/denoise_time.py): the tiles save 0.06 / 0.05 / 0.04 / 0.02 ms at steps 1 / 2 / 4 / 8 and nothing at
// step 16, where a residue class's lattice is down to 50 x 38 points and the strided staging costs what the reuse saves; beyond,
// the lattices no longer fill a tile.  FLUX_DENOISE_LDS_LEVELS overrides the default for that measurement; the two kernels
// compute the same bits.
constexpr int kDefaultLdsLevels = 4;

// f: the sigmas of resolve_params.  d_in: the [H][W][3] frame of flux_denoise, or, `moments`, the [H][W][FLUX_MOMENT_CHANNELS] buffer
// of flux_denoise_moments.
static hipError_t launch(Frame f, int levels, bool moments, uint64_t width, uint64_t height, const double *d_in, const double *d_aov,
                         double *d_out, double *d_work, hipStream_t stream) {
    f.W = (int32_t)width;
    f.H = (int32_t)height;
    f.tiles_x = (int32_t)((width + kTileW - 1) / kTileW);
    f.npix = (size_t)(width * height);
    f.work = d_work;
    f.step = 1;
    // (at most 2^26 / 8 tiles of one column: far inside a 1-D grid)
    const dim3 grid((uint32_t)((uint64_t)f.tiles_x * ((height + kTileH - 1) / kTileH))), block(kTileW * kTileH);
    if (moments) {
        hipLaunchKernelGGL(denoise_pack_kernel<true>, grid, block, 0, stream, f, d_in, d_aov);
        hipLaunchKernelGGL(denoise_varfilter_kernel, grid, block, 0, stream, f);
    } else {
        hipLaunchKernelGGL(denoise_pack_kernel<false>, grid, block, 0, stream, f, d_in, d_aov);
        hipLaunchKernelGGL(denoise_variance_kernel, grid, block, 0, stream, f);
    }
    const int lds_levels = denoise_lds_levels(kDefaultLdsLevels);
    const int in_stride = moments ? FLUX_MOMENT_CHANNELS : 3;
    for (int k = 0; k < levels; k++) {
        f.step = 1 << k;
        const int src = (k & 1) ? 11 : 7, dst = (k & 1) ? 7 : 11;
        const bool last = k == levels - 1;
        if (k < lds_levels) {
            // the lattice of the largest residue class (alpha = beta = 0), in tiles
            const uint64_t lat_w = (width + f.step - 1) / f.step, lat_h = (height + f.step - 1) / f.step;
            const uint64_t ltx = (lat_w + kTileW - 1) / kTileW, lty = (lat_h + kTileH - 1) / kTileH;
            const dim3 lgrid((uint32_t)(ltx * lty), (uint32_t)(f.step * f.step));  // (y: at most 128^2)
            if (last)
                hipLaunchKernelGGL(denoise_level_lds_kernel<true>, lgrid, block, 0, stream, f, src, dst, (int)ltx, d_in, d_out, in_stride);
            else
                hipLaunchKernelGGL(denoise_level_lds_kernel<false>, lgrid, block, 0, stream, f, src, dst, (int)ltx, d_in, d_out, in_stride);
        } else if (last) {
            hipLaunchKernelGGL(denoise_level_kernel<true>, grid, block, 0, stream, f, src, dst, d_in, d_out, in_stride);
        } else {
            hipLaunchKernelGGL(denoise_level_kernel<false>, grid, block, 0, stream, f, src, dst, d_in, d_out, in_stride);
        }
    }
    return hipGetLastError();
}

// flux_denoise_device and flux_denoise_moments_device as `fn`, whose input pointer the header calls `in_name`.  The refusals come in
// the header's order: size, null pointer, params, work_doubles, aliasing, device.
static int device_call(const char *fn, const char *in_name, bool moments, int device, uint64_t width, uint64_t height, void *d_in, void *d_aov,
                       const double *params, void *d_out_rgb, void *d_work, uint64_t work_doubles, void *hip_stream) {
    if (int rc = check_size(width, height)) return rc;
    if (!d_in || !d_aov || !d_out_rgb || !d_work) return fail(FLUX_E_INVALID, "%s: null device pointer", fn);
    Frame f{};
    int levels;
    if (int rc = resolve_params(params, levels, f)) return rc;
    const uint64_t need = flux_denoise_work_doubles(width, height);
    if (work_doubles < need)
        return fail(FLUX_E_INVALID, "%s: work_doubles %llu is below flux_denoise_work_doubles = %llu", fn, (unsigned long long)work_doubles,
                    (unsigned long long)need);
    if (d_out_rgb == d_in || d_out_rgb == d_work)
        return fail(FLUX_E_INVALID, "%s: d_out_rgb must be neither %s nor d_work (unusable pixels are copied from %s by the last launch)", fn,
                    in_name, in_name);
    if (int rc = check_device(device)) return rc;
    DeviceGuard guard(device);
    if (!guard.ok) return fail(FLUX_E_DEVICE, "hipSetDevice(%d) failed", device);
    HIP_TRY(launch(f, levels, moments, width, height, (const double *)d_in, (const double *)d_aov, (double *)d_out_rgb, (double *)d_work,
                   (hipStream_t)hip_stream));
    return FLUX_OK;
}

// flux_denoise and flux_denoise_moments as `fn`: `in` is [H][W][in_channels] on the host.
static int host_call(const char *fn, bool moments, int device, uint64_t width, uint64_t height, const double *in, const double *aov,
                     const double *params, double *out_rgb) {
    if (int rc = check_size(width, height)) return rc;
    if (!in || !aov || !out_rgb) return fail(FLUX_E_INVALID, "%s: null pointer", fn);
    Frame f{};
    int levels;
    if (int rc = resolve_params(params, levels, f)) return rc;
    if (int rc = check_device(device)) return rc;
    DeviceGuard guard(device);
    if (!guard.ok) return fail(FLUX_E_DEVICE, "hipSetDevice(%d) failed", device);
    const size_t npix = (size_t)(width * height), in_doubles = npix * (moments ? FLUX_MOMENT_CHANNELS : 3);
    DevBuf<double> d_in, d_aov, d_out, d_work;  // released with `device` still current (guard is older)
    HIP_TRY(d_in.alloc(in_doubles));
    HIP_TRY(d_aov.alloc(npix * FLUX_AOV_CHANNELS));
    HIP_TRY(d_out.alloc(npix * 3));
    HIP_TRY(d_work.alloc((size_t)flux_denoise_work_doubles(width, height)));
    HIP_TRY(hipMemcpy(d_in, in, in_doubles * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_aov, aov, npix * FLUX_AOV_CHANNELS * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(launch(f, levels, moments, width, height, d_in, d_aov, d_out, d_work, nullptr));
    HIP_TRY(hipMemcpy(out_rgb, d_out, npix * 3 * sizeof(double), hipMemcpyDeviceToHost));  // (synchronises with the null stream)
    return FLUX_OK;
}

}  // namespace denoise
}  // namespace flux

namespace dn = flux::denoise;

extern "C" {

uint64_t flux_denoise_work_doubles(uint64_t width, uint64_t height) {
    if (width == 0 || height == 0 || width > dn::kMaxPixels || height > dn::kMaxPixels || width * height > dn::kMaxPixels) return 0;
    return (uint64_t)dn::kPlanes * width * height;
}

int flux_denoise_device(int device, uint64_t width, uint64_t height, void *d_rgb, void *d_aov, const double *params, void *d_out_rgb,
                        void *d_work, uint64_t work_doubles, void *hip_stream) {
    return dn::device_call("flux_denoise_device", "d_rgb", false, device, width, height, d_rgb, d_aov, params, d_out_rgb, d_work,
                           work_doubles, hip_stream);
}

int flux_denoise_moments_device(int device, uint64_t width, uint64_t height, void *d_moments, void *d_aov, const double *params,
                                void *d_out_rgb, void *d_work, uint64_t work_doubles, void *hip_stream) {
    return dn::device_call("flux_denoise_moments_device", "d_moments", true, device, width, height, d_moments, d_aov, params, d_out_rgb,
                           d_work, work_doubles, hip_stream);
}

int flux_denoise(int device, uint64_t width, uint64_t height, const double *rgb, const double *aov, const double *params,
                 double *out_rgb) {
    return dn::host_call("flux_denoise", false, device, width, height, rgb, aov, params, out_rgb);
}

int flux_denoise_moments(int device, uint64_t width, uint64_t height, const double *moments, const double *aov, const double *params,
                         double *out_rgb) {
    return dn::host_call("flux_denoise_moments", true, device, width, height, moments, aov, params, out_rgb);
}

}  // extern "C"
