// denoise.hip -- flux_denoise*: the feature-guided a-trous filter of include/flux_abi.h over a frame of
// flux_render_rows and the feature buffers of flux_render_aov_rows.  tests/denoise_spec.py states the same filter in numpy.
//
// Its own translation unit under the build's default flags (-ffp-contract=off): every sum and product below keeps the order the
// header gives it, division and sqrt are IEEE, and the one function that differs from the numpy statement is fexp2 (flux_math.h).
//
// Three kernels, all one thread per pixel in blocks of 32 x 8 pixels (four 64-lane waves, each two image rows of 32 pixels); the
// measured-variance path of flux_denoise_moments* adds three small ones of the same shape, stated where they stand:
//   denoise_pack_kernel      AoS rgb + aov -> planes of W*H doubles: albedo (3), normal (3), depth, colour (3).  An unusable pixel
//                            gets a NaN depth: no usable pixel has one, so the depth plane doubles as the usable flag.
//   denoise_variance_kernel  the guide-weighted variance of the luminance over 5 x 5, two passes over weights kept in registers.
//   denoise_level_kernel     one a-trous level, launched `levels` times between two colour + variance plane sets (never in place);
//                            the last launch writes the AoS frame with max_to_one and copies the unusable pixels from the input.
//                            Steps 1-8 run as denoise_level_lds_kernel (one residue class of the step's lattice per block, staged
//                            in LDS), larger steps as plain global gathers: launch() has the measurement behind the choice.
// The luminance is recomputed from the colour wherever it is needed (three operations, the same bits as a stored plane).
// No atomics, a fixed tap order: bit-reproducible.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>

#include "../../include/flux_abi.h"
#include "flux_ctx.h"
#include "flux_math.h"

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

struct Params {
    int levels;
    double sigma_l, sn2, sz2, sa2;  // sigma_n^2, sigma_z^2, sigma_a^2: one rounding each, as the numpy statement
};

struct Frame {
    int32_t W, H, tiles_x;
    int32_t step;
    size_t npix;
    double *work;  // kPlanes planes of npix doubles
    double sigma_l, sn2, sz2, sa2;
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

__global__ __launch_bounds__(kTileW *kTileH) void denoise_pack_kernel(Frame f, const double *__restrict__ rgb,
                                                                      const double *__restrict__ aov) {
    int x, y;
    if (!my_pixel(f, x, y)) return;
    const size_t idx = (size_t)y * f.W + x;
    const double *c = rgb + idx * 3;
    const double *g = aov + idx * FLUX_AOV_CHANNELS;
    bool ok = finite(c[0]) && finite(c[1]) && finite(c[2]) && finite(lum(c[0], c[1], c[2]));
    for (int k = 0; k < 6; k++) ok = ok && finite(g[k]);
    const double z = g[FLUX_AOV_DEPTH];
    ok = ok && z == z;
    for (int k = 0; k < 6; k++) f.work[k * f.npix + idx] = g[k];
    f.work[6 * f.npix + idx] = ok ? z : __builtin_nan("");
    for (int k = 0; k < 3; k++) f.work[(7 + k) * f.npix + idx] = c[k];
}

__global__ __launch_bounds__(kTileW *kTileH) void denoise_variance_kernel(Frame f) {
    int x, y;
    if (!my_pixel(f, x, y)) return;
    const size_t idx = (size_t)y * f.W + x;
    const double *work = f.work;
    const double zp = work[6 * f.npix + idx];
    if (zp != zp) return;  // unusable: no tap ever reads its variance
    const Guide p = load_guide(work, f.npix, idx, zp);
    double w[25], l[25];
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int j = -kHalo; j <= kHalo; j++) {
#pragma unroll
        for (int i = -kHalo; i <= kHalo; i++) {
            const int t = (j + kHalo) * 5 + (i + kHalo);
            const int qx = x + i, qy = y + j;
            w[t] = -1.0;  // a skipped tap
            l[t] = 0.0;
            if (qx < 0 || qx >= f.W || qy < 0 || qy >= f.H) continue;
            const size_t q = (size_t)qy * f.W + qx;
            const double zq = work[6 * f.npix + q];
            if (zq != zq) continue;
            const Guide g = load_guide(work, f.npix, q, zq);
            w[t] = fastmath::fexp2(-__builtin_fmin(guide_exponent(p, g, f), kEMax));
            l[t] = lum(work[7 * f.npix + q], work[8 * f.npix + q], work[9 * f.npix + q]);
            s0 += w[t];
            s1 += w[t] * l[t];
        }
    }
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

// ---- the measured-variance path (flux_denoise_moments*) -----------------------------------------------------
// The same planes and the same level kernels; what differs is where a pixel's variance comes from:
//   denoise_pack_moments_kernel  denoise_pack_kernel over the moments buffer ([H][W][8]: rgb = channels 0-2, v = channel 3): a pixel is
//                                usable only if v is finite and >= 0 as well, and v goes to the SECOND set's variance plane (14),
//                                which no launch reads before the first level has written it.
//   denoise_varfilter_kernel     var_p = sum w v_q / sum w over the step-1 taps, w from the guides alone, one pass: plane 14 -> plane 10.
//   denoise_unusable_kernel      the level kernels copy an unusable pixel from a [H][W][3] frame, which the moments buffer is not: just
//                                before the last level this kernel writes the unusable pixels' rgb as such a frame into the colour
//                                planes of the set the last level does not read (and, being the last, does not write).
__global__ __launch_bounds__(kTileW *kTileH) void denoise_pack_moments_kernel(Frame f, const double *__restrict__ mom,
                                                                              const double *__restrict__ aov) {
    int x, y;
    if (!my_pixel(f, x, y)) return;
    const size_t idx = (size_t)y * f.W + x;
    const double *c = mom + idx * FLUX_MOMENT_CHANNELS;
    const double *g = aov + idx * FLUX_AOV_CHANNELS;
    const double v = c[FLUX_MOMENT_VAR];
    bool ok = finite(c[0]) && finite(c[1]) && finite(c[2]) && finite(lum(c[0], c[1], c[2])) && finite(v) && v >= 0.0;
    for (int k = 0; k < 6; k++) ok = ok && finite(g[k]);
    const double z = g[FLUX_AOV_DEPTH];
    ok = ok && z == z;
    for (int k = 0; k < 6; k++) f.work[k * f.npix + idx] = g[k];
    f.work[6 * f.npix + idx] = ok ? z : __builtin_nan("");
    for (int k = 0; k < 3; k++) f.work[(7 + k) * f.npix + idx] = c[k];
    f.work[14 * f.npix + idx] = v;
}

__global__ __launch_bounds__(kTileW *kTileH) void denoise_varfilter_kernel(Frame f) {
    int x, y;
    if (!my_pixel(f, x, y)) return;
    const size_t idx = (size_t)y * f.W + x;
    const double *work = f.work;
    const double zp = work[6 * f.npix + idx];
    if (zp != zp) return;  // unusable: no tap ever reads its variance
    const Guide p = load_guide(work, f.npix, idx, zp);
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int j = -kHalo; j <= kHalo; j++) {
#pragma unroll
        for (int i = -kHalo; i <= kHalo; i++) {
            const int qx = x + i, qy = y + j;
            if (qx < 0 || qx >= f.W || qy < 0 || qy >= f.H) continue;
            const size_t q = (size_t)qy * f.W + qx;
            const double zq = work[6 * f.npix + q];
            if (zq != zq) continue;
            const double w = fastmath::fexp2(-__builtin_fmin(guide_exponent(p, load_guide(work, f.npix, q, zq), f), kEMax));
            s0 += w;
            s1 += w * work[14 * f.npix + q];
        }
    }
    f.work[10 * f.npix + idx] = s1 / s0;
}

__global__ __launch_bounds__(kTileW *kTileH) void denoise_unusable_kernel(Frame f, int dst, const double *__restrict__ mom) {
    int x, y;
    if (!my_pixel(f, x, y)) return;
    const size_t idx = (size_t)y * f.W + x;
    const double zp = f.work[6 * f.npix + idx];
    if (zp == zp) return;
    double *frame = f.work + (size_t)dst * f.npix;  // 3 npix doubles, [H][W][3]
    for (int k = 0; k < 3; k++) frame[idx * 3 + k] = mom[idx * FLUX_MOMENT_CHANNELS + k];
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

// One level by global gathers: colour + variance planes `src` (7: set A, 11: set B) -> `dst`, or, LAST, the AoS frame `out`.  A block is
// a dense 32 x 8 tile of the image: every tap is one coalesced 256-B read per image row of the wave, served by the caches.
template <bool LAST>
__global__ __launch_bounds__(kTileW *kTileH) void denoise_level_kernel(Frame f, int src, int dst, const double *__restrict__ rgb_in,
                                                                       double *__restrict__ out) {
    int x, y;
    if (!my_pixel(f, x, y)) return;
    const size_t idx = (size_t)y * f.W + x;
    const double *work = f.work;
    const double zp = work[6 * f.npix + idx];
    if (zp != zp) {  // unusable: bit for bit from the input, and nothing of it in the planes is ever read
        if (LAST)
            for (int k = 0; k < 3; k++) out[idx * 3 + k] = rgb_in[idx * 3 + k];
        return;
    }
    const Guide p = load_guide(work, f.npix, idx, zp);
    const double *c0 = work + (size_t)src * f.npix, *c1 = c0 + f.npix, *c2 = c1 + f.npix, *var = c2 + f.npix;
    const double lp = lum(c0[idx], c1[idx], c2[idx]);
    const double sd = f.sigma_l * __builtin_sqrt(var[idx]) + kSdFloor;
    Sums s;
#pragma unroll
    for (int j = -kHalo; j <= kHalo; j++) {
        const int qy = y + j * f.step;
        if (qy < 0 || qy >= f.H) continue;
#pragma unroll
        for (int i = -kHalo; i <= kHalo; i++) {
            const int qx = x + i * f.step;
            if (qx < 0 || qx >= f.W) continue;
            const size_t q = (size_t)qy * f.W + qx;
            const double zq = work[6 * f.npix + q];
            if (zq != zq) continue;
            add_tap(s, p, load_guide(work, f.npix, q, zq), lp, sd, kH5[j + kHalo] * kH5[i + kHalo], c0[q], c1[q], c2[q], var[q], f);
        }
    }
    store_pixel<LAST>(s, f, idx, dst, out);
}

// The same level through LDS.  A step-s pass is s^2 independent dense 5 x 5 filters, one per residue class (x = alpha, y = beta mod s):
// a block takes 32 x 8 points of ONE class's lattice, stages them and their halo of 2 (36 x 12 points x 11 doubles = 38 016 B, one
// plane per quantity, so a wave's tap is two conflict-free runs of 32 consecutive doubles) and reads every tap from there.  Points off
// the image are staged with a NaN depth, the mark of a pixel no tap may use.  blockIdx.y = beta * s + alpha; blockIdx.x = the tile within
// the largest class's lattice (classes with a shorter lattice leave their last tiles empty).  Global reads and writes are s doubles apart.
constexpr int kLdsW = kTileW + 2 * kHalo, kLdsH = kTileH + 2 * kHalo, kLdsPoints = kLdsW * kLdsH, kLdsPlanes = 11;
template <bool LAST>
__global__ __launch_bounds__(kTileW *kTileH) void denoise_level_lds_kernel(Frame f, int src, int dst, int lat_tiles_x,
                                                                           const double *__restrict__ rgb_in, double *__restrict__ out) {
    __shared__ double tile[kLdsPlanes][kLdsPoints];  // 0-2 albedo, 3-5 normal, 6 depth, 7-9 colour, 10 variance
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
    const size_t idx = (size_t)y * f.W + (size_t)x;
    const int centre = (ty + kHalo) * kLdsW + tx + kHalo;
    const double zp = tile[6][centre];
    if (zp != zp) {
        if (LAST)
            for (int k = 0; k < 3; k++) out[idx * 3 + k] = rgb_in[idx * 3 + k];
        return;
    }
    auto guide_at = [&](int t, double z) {
        Guide g;
        g.a0 = tile[0][t];
        g.a1 = tile[1][t];
        g.a2 = tile[2][t];
        g.n0 = tile[3][t];
        g.n1 = tile[4][t];
        g.n2 = tile[5][t];
        g.z = z;
        return g;
    };
    const Guide p = guide_at(centre, zp);
    const double lp = lum(tile[7][centre], tile[8][centre], tile[9][centre]);
    const double sd = f.sigma_l * __builtin_sqrt(tile[10][centre]) + kSdFloor;
    Sums sums;
#pragma unroll
    for (int j = -kHalo; j <= kHalo; j++) {
#pragma unroll
        for (int i = -kHalo; i <= kHalo; i++) {
            const int t = centre + j * kLdsW + i;
            const double zq = tile[6][t];
            if (zq != zq) continue;
            add_tap(sums, p, guide_at(t, zq), lp, sd, kH5[j + kHalo] * kH5[i + kHalo], tile[7][t], tile[8][t], tile[9][t], tile[10][t], f);
        }
    }
    store_pixel<LAST>(sums, f, idx, dst, out);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------

static bool positive_finite(double x) { return std::isfinite(x) && x > 0.0; }

// params (or the defaults for nullptr) -> p; FLUX_E_INVALID for a value the header rules out
static int resolve_params(const double *params, Params &p) {
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
    p.levels = (int)v[0];
    p.sigma_l = v[1];
    p.sn2 = v[2] * v[2];
    p.sz2 = v[3] * v[3];
    p.sa2 = v[4] * v[4];
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
static int lds_levels() {
    const char *e = std::getenv("FLUX_DENOISE_LDS_LEVELS");
    return e ? std::atoi(e) : kDefaultLdsLevels;
}

// d_rgb: the [H][W][3] frame of flux_denoise, or, `moments`, the [H][W][FLUX_MOMENT_CHANNELS] buffer of flux_denoise_moments
static hipError_t launch(const Params &p, uint64_t width, uint64_t height, const double *d_rgb, const double *d_aov, double *d_out,
                         double *d_work, hipStream_t stream, bool moments = false) {
    Frame f{};
    f.W = (int32_t)width;
    f.H = (int32_t)height;
    f.tiles_x = (int32_t)((width + kTileW - 1) / kTileW);
    f.npix = (size_t)(width * height);
    f.work = d_work;
    f.sigma_l = p.sigma_l;
    f.sn2 = p.sn2;
    f.sz2 = p.sz2;
    f.sa2 = p.sa2;
    f.step = 1;
    // (at most 2^26 / 8 tiles of one column: far inside a 1-D grid)
    const dim3 grid((uint32_t)((uint64_t)f.tiles_x * ((height + kTileH - 1) / kTileH))), block(kTileW * kTileH);
    if (moments) {
        hipLaunchKernelGGL(denoise_pack_moments_kernel, grid, block, 0, stream, f, d_rgb, d_aov);
        hipLaunchKernelGGL(denoise_varfilter_kernel, grid, block, 0, stream, f);
    } else {
        hipLaunchKernelGGL(denoise_pack_kernel, grid, block, 0, stream, f, d_rgb, d_aov);
        hipLaunchKernelGGL(denoise_variance_kernel, grid, block, 0, stream, f);
    }
    for (int k = 0; k < p.levels; k++) {
        f.step = 1 << k;
        const int src = (k & 1) ? 11 : 7, dst = (k & 1) ? 7 : 11;
        const bool last = k == p.levels - 1;
        if (last && moments) {  // the frame the last level copies its unusable pixels from: in the set it neither reads nor writes
            hipLaunchKernelGGL(denoise_unusable_kernel, grid, block, 0, stream, f, dst, d_rgb);
            d_rgb = d_work + (size_t)dst * f.npix;
        }
        if (k < lds_levels()) {
            // the lattice of the largest residue class (alpha = beta = 0), in tiles
            const uint64_t lat_w = (width + f.step - 1) / f.step, lat_h = (height + f.step - 1) / f.step;
            const uint64_t ltx = (lat_w + kTileW - 1) / kTileW, lty = (lat_h + kTileH - 1) / kTileH;
            const dim3 lgrid((uint32_t)(ltx * lty), (uint32_t)(f.step * f.step));  // (y: at most 128^2)
            if (last)
                hipLaunchKernelGGL(denoise_level_lds_kernel<true>, lgrid, block, 0, stream, f, src, dst, (int)ltx, d_rgb, d_out);
            else
                hipLaunchKernelGGL(denoise_level_lds_kernel<false>, lgrid, block, 0, stream, f, src, dst, (int)ltx, d_rgb, d_out);
        } else if (last) {
            hipLaunchKernelGGL(denoise_level_kernel<true>, grid, block, 0, stream, f, src, dst, d_rgb, d_out);
        } else {
            hipLaunchKernelGGL(denoise_level_kernel<false>, grid, block, 0, stream, f, src, dst, d_rgb, d_out);
        }
    }
    return hipGetLastError();
}

}  // namespace denoise
}  // namespace flux

using flux::fail;
namespace dn = flux::denoise;

extern "C" {

uint64_t flux_denoise_work_doubles(uint64_t width, uint64_t height) {
    if (width == 0 || height == 0 || width > dn::kMaxPixels || height > dn::kMaxPixels || width * height > dn::kMaxPixels) return 0;
    return (uint64_t)dn::kPlanes * width * height;
}

int flux_denoise_device(int device, uint64_t width, uint64_t height, void *d_rgb, void *d_aov, const double *params, void *d_out_rgb,
                        void *d_work, uint64_t work_doubles, void *hip_stream) {
    if (int rc = dn::check_size(width, height)) return rc;
    if (!d_rgb || !d_aov || !d_out_rgb || !d_work) return fail(FLUX_E_INVALID, "flux_denoise_device: null device pointer");
    dn::Params p;
    if (int rc = dn::resolve_params(params, p)) return rc;
    if (work_doubles < flux_denoise_work_doubles(width, height))
        return fail(FLUX_E_INVALID, "flux_denoise_device: work_doubles %llu is below flux_denoise_work_doubles = %llu",
                    (unsigned long long)work_doubles, (unsigned long long)flux_denoise_work_doubles(width, height));
    if (d_out_rgb == d_rgb || d_out_rgb == d_work)
        return fail(FLUX_E_INVALID, "flux_denoise_device: d_out_rgb must be neither d_rgb nor d_work (unusable pixels are copied from d_rgb "
                                    "by the last launch)");
    if (int rc = flux::check_device(device)) return rc;
    flux::DeviceGuard guard(device);
    if (!guard.ok) return fail(FLUX_E_DEVICE, "hipSetDevice(%d) failed", device);
    HIP_TRY(dn::launch(p, width, height, (const double *)d_rgb, (const double *)d_aov, (double *)d_out_rgb, (double *)d_work,
                       (hipStream_t)hip_stream));
    return FLUX_OK;
}

int flux_denoise_moments_device(int device, uint64_t width, uint64_t height, void *d_moments, void *d_aov, const double *params,
                                void *d_out_rgb, void *d_work, uint64_t work_doubles, void *hip_stream) {
    if (int rc = dn::check_size(width, height)) return rc;
    if (!d_moments || !d_aov || !d_out_rgb || !d_work) return fail(FLUX_E_INVALID, "flux_denoise_moments_device: null device pointer");
    dn::Params p;
    if (int rc = dn::resolve_params(params, p)) return rc;
    if (work_doubles < flux_denoise_work_doubles(width, height))
        return fail(FLUX_E_INVALID, "flux_denoise_moments_device: work_doubles %llu is below flux_denoise_work_doubles = %llu",
                    (unsigned long long)work_doubles, (unsigned long long)flux_denoise_work_doubles(width, height));
    if (d_out_rgb == d_moments || d_out_rgb == d_work)
        return fail(FLUX_E_INVALID, "flux_denoise_moments_device: d_out_rgb must be neither d_moments nor d_work");
    if (int rc = flux::check_device(device)) return rc;
    flux::DeviceGuard guard(device);
    if (!guard.ok) return fail(FLUX_E_DEVICE, "hipSetDevice(%d) failed", device);
    HIP_TRY(dn::launch(p, width, height, (const double *)d_moments, (const double *)d_aov, (double *)d_out_rgb, (double *)d_work,
                       (hipStream_t)hip_stream, true));
    return FLUX_OK;
}

int flux_denoise_moments(int device, uint64_t width, uint64_t height, const double *moments, const double *aov, const double *params,
                         double *out_rgb) {
    if (int rc = dn::check_size(width, height)) return rc;
    if (!moments || !aov || !out_rgb) return fail(FLUX_E_INVALID, "flux_denoise_moments: null pointer");
    dn::Params p;
    if (int rc = dn::resolve_params(params, p)) return rc;
    if (int rc = flux::check_device(device)) return rc;
    flux::DeviceGuard guard(device);
    if (!guard.ok) return fail(FLUX_E_DEVICE, "hipSetDevice(%d) failed", device);
    const size_t npix = (size_t)(width * height);
    flux::DevBuf<double> d_mom, d_aov, d_out, d_work;  // released with `device` still current (guard is older)
    HIP_TRY(d_mom.alloc(npix * FLUX_MOMENT_CHANNELS));
    HIP_TRY(d_aov.alloc(npix * FLUX_AOV_CHANNELS));
    HIP_TRY(d_out.alloc(npix * 3));
    HIP_TRY(d_work.alloc((size_t)flux_denoise_work_doubles(width, height)));
    HIP_TRY(hipMemcpy(d_mom, moments, npix * FLUX_MOMENT_CHANNELS * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_aov, aov, npix * FLUX_AOV_CHANNELS * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(dn::launch(p, width, height, d_mom, d_aov, d_out, d_work, nullptr, true));
    HIP_TRY(hipMemcpy(out_rgb, d_out, npix * 3 * sizeof(double), hipMemcpyDeviceToHost));  // (synchronises with the null stream)
    return FLUX_OK;
}

int flux_denoise(int device, uint64_t width, uint64_t height, const double *rgb, const double *aov, const double *params,
                 double *out_rgb) {
    if (int rc = dn::check_size(width, height)) return rc;
    if (!rgb || !aov || !out_rgb) return fail(FLUX_E_INVALID, "flux_denoise: null pointer");
    dn::Params p;
    if (int rc = dn::resolve_params(params, p)) return rc;
    if (int rc = flux::check_device(device)) return rc;
    flux::DeviceGuard guard(device);
    if (!guard.ok) return fail(FLUX_E_DEVICE, "hipSetDevice(%d) failed", device);
    const size_t npix = (size_t)(width * height);
    flux::DevBuf<double> d_rgb, d_aov, d_out, d_work;  // released with `device` still current (guard is older)
    HIP_TRY(d_rgb.alloc(npix * 3));
    HIP_TRY(d_aov.alloc(npix * FLUX_AOV_CHANNELS));
    HIP_TRY(d_out.alloc(npix * 3));
    HIP_TRY(d_work.alloc((size_t)flux_denoise_work_doubles(width, height)));
    HIP_TRY(hipMemcpy(d_rgb, rgb, npix * 3 * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_aov, aov, npix * FLUX_AOV_CHANNELS * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(dn::launch(p, width, height, d_rgb, d_aov, d_out, d_work, nullptr));
    HIP_TRY(hipMemcpy(out_rgb, d_out, npix * 3 * sizeof(double), hipMemcpyDeviceToHost));  // (synchronises with the null stream)
    return FLUX_OK;
}

}  // extern "C"
