// flux_moments.h -- the moments layout (include/flux_abi.h FLUX_MOMENT_*) from a pixel's five sums: the ONLY
// statement of the epilogue's operation order.  moments_kernel (moments_body.inc, all three copies of render.hip) calls it with
// (N, RenderParams::pixel_denom), adaptive_finish_kernel (adaptive.hip) with (N c, 1 / (N c)); a pixel that took one pass gets the
// same bits from both (1.0 / N is pixel_denom bit for bit).
#pragma once
#include <hip/hip_runtime.h>

namespace flux {

// Value ch of v0, v1, ...: the channel a lane stores, as a chain of selects over values.  (Handed an array, the compiler turned the
// chain into an indexed load and kept the array in scratch.)
template <class... V>
__device__ __forceinline__ double pick(uint32_t ch, double v0, V... v) {
    double r = v0;
    uint32_t k = 0;
    ((r = ch == ++k ? v : r), ...);
    return r;
}

// With n = count samples, L a sample's radiance and l = (0.2126 L.r + 0.7152 L.g) + 0.0722 L.b its luminance:
//   mean  = sum c * denom                                               out[4..6] (FLUX_MOMENT_MEAN), unclamped
//   rgb   = max_to_one(mean), finish_pixel's operations in its order     out[0..2] (FLUX_MOMENT_RGB); color.rs:35-44
//   s2    = max(0, sum l^2 - (sum l * sum l) / n) / (n - 1)              out[7] (FLUX_MOMENT_S2); the max keeps a NaN
//   var   = (s2 / n) * (k * k), k = 1 / max(mean) where that exceeds 1   out[3] (FLUX_MOMENT_VAR): the variance of lum(rgb)
// Nothing else is clamped: a NaN or inf sample shows in out[3] and out[7].  No expression here has a product feeding a sum, so
// contract(fast) has nothing to fuse; the pragma says so in code, for the copies of render.hip compiled under it.
__device__ __forceinline__ void moments_of_sums(double sum_r, double sum_g, double sum_b, double sum_l, double sum_l2, double count,
                                                double denom, double (&out)[8]) {
#pragma clang fp contract(off)
    const double mr = sum_r * denom, mg = sum_g * denom, mb = sum_b * denom;
    double r = mr, g = mg, b = mb, k = 1.0;
    const double mx1 = r > g ? r : g;
    const double mx2 = mx1 > b ? mx1 : b;
    if (mx2 > 1.0) {
        k = 1.0 / mx2;
        r *= k;
        g *= k;
        b *= k;
    }
    const double d = sum_l2 - (sum_l * sum_l) / count;
    const double s2 = (d < 0.0 ? 0.0 : d) / (count - 1.0);  // (a NaN stays a NaN)
    out[0] = r;
    out[1] = g;
    out[2] = b;
    out[3] = (s2 / count) * (k * k);
    out[4] = mr;
    out[5] = mg;
    out[6] = mb;
    out[7] = s2;
}

}  // namespace flux
