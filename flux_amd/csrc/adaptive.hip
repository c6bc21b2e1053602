// adaptive.hip -- what the adaptive sampler (include/flux_abi.h flux_render_adaptive_rows*) runs between and
// after its passes: which pixels take the next pass, and the per-pixel state turned into the moments layout.  tests/adaptive_spec.py
// states the same rule in numpy.  The pass itself traces paths and lives with the render kernels (adaptive_body.inc).
//
// Its own translation unit under the build's default flags (-ffp-contract=off): no lobe code, every operation below is IEEE and
// keeps the order the header gives it, in the STRICT and the FAST arithmetic alike.
//
// Four kernels, one thread per pixel in 256-thread blocks (adaptive_finish_kernel: eight threads per pixel; adaptive_count_kernel: a
// grid-stride loop):
//   adaptive_hot_kernel     hot[p] = e2 > tau2 from the pixel's running sums (a NaN is never hot, an inf is).
//   adaptive_select_kernel  active[p] = any hot pixel within Chebyshev distance `dilate`, clipped at the call's edges; the active
//                           pixels are compacted into the work list with a wave ballot, the block's sixteen ballot counts added up
//                           through LDS, and ONE vector atomic add per 1024-pixel block on the counter (a wave's lanes then take
//                           consecutive slots behind the block's earlier waves by their rank in the ballot).  The list's order
//                           depends on which block's atomic lands first; no output bit depends on it, since a pass reads and
//                           writes the state of its own pixel only.
//   adaptive_finish_kernel  the moments layout of the state with n = N c for N, one 64-byte line per pixel (a double per thread),
//                           and the pass map.
//   adaptive_count_kernel   the number of pixels with c == max_passes, for the call's `info` alone: at most 64 blocks stride over the
//                           pass counts and each wave adds its sum once.  (Counted in the finish kernel, one atomic add per wave on
//                           ONE address, a frame whose every pixel is at the limit cost 0.7 ms at 800 x 600: 60 000 serialised adds.)
#include <hip/hip_runtime.h>

#include "flux_moments.h"
#include "flux_tables.h"

namespace flux {
namespace adaptive {

constexpr unsigned kBlock = 256;

__global__ __launch_bounds__(kBlock) void adaptive_hot_kernel(AdaptiveRule R, uint64_t pixels, const double *__restrict__ sums,
                                                             const uint32_t *__restrict__ passes, unsigned char *__restrict__ hot) {
    const uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= pixels) return;
    const double sl = sums[p * kAdaptiveSums + 3], sl2 = sums[p * kAdaptiveSums + 4];
    const double n = (double)((uint64_t)R.nsamp * passes[p]);
    const double m = sl / n;
    const double d = sl2 - (sl * sl) / n;
    const double s2 = (d < 0.0 ? 0.0 : d) / (n - 1.0);  // (a NaN stays a NaN)
    const double mm = m > R.lum_floor ? m : R.lum_floor;
    const double e2 = (s2 / n) / (mm * mm);
    hot[p] = e2 > R.tau2 ? 1 : 0;  // (false for a NaN)
}

constexpr unsigned kSelectBlock = 1024, kSelectWaves = kSelectBlock / 64;
__global__ __launch_bounds__(kSelectBlock) void adaptive_select_kernel(uint32_t rows, uint32_t width, int dilate,
                                                                const unsigned char *__restrict__ hot, uint32_t *__restrict__ list,
                                                                uint32_t *__restrict__ count) {
    const uint64_t pixels = (uint64_t)rows * width;
    const uint64_t p = (uint64_t)blockIdx.x * kSelectBlock + threadIdx.x;
    __shared__ uint32_t wave_count[kSelectWaves];
    __shared__ uint32_t block_base;
    bool active = false;
    if (p < pixels) {
        const int y = (int)(p / width), x = (int)(p - (uint64_t)y * width);
        const int y0 = y - dilate < 0 ? 0 : y - dilate, y1 = y + dilate > (int)rows - 1 ? (int)rows - 1 : y + dilate;
        const int x0 = x - dilate < 0 ? 0 : x - dilate, x1 = x + dilate > (int)width - 1 ? (int)width - 1 : x + dilate;
        for (int yy = y0; yy <= y1; ++yy)
            for (int xx = x0; xx <= x1; ++xx) active |= hot[(size_t)yy * width + xx] != 0;
    }
    const unsigned long long mask = __ballot(active);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0u) wave_count[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t total = 0;
        for (unsigned w = 0; w < kSelectWaves; ++w) total += wave_count[w];
        block_base = total != 0u ? atomicAdd(count, total) : 0u;
    }
    __syncthreads();
    if (active) {
        uint32_t base = block_base;
        for (uint32_t w = 0; w < wave; ++w) base += wave_count[w];
        list[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = (uint32_t)p;
    }
}

__global__ __launch_bounds__(kBlock) void adaptive_finish_kernel(uint32_t nsamp, uint64_t pixels, const double *__restrict__ sums,
                                                                const uint32_t *__restrict__ passes, double *__restrict__ out,
                                                                uint32_t *__restrict__ out_passes) {
    const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t p = t >> 3;
    const uint32_t ch = (uint32_t)t & 7u;
    if (p < pixels) {
        const double *s = sums + p * kAdaptiveSums;
        const uint32_t c = passes[p];
        const double count = (double)((uint64_t)nsamp * c);
        double m[8];  // (IEEE: with c = 1 the denominator is the host's RenderParams::pixel_denom bit for bit)
        moments_of_sums(s[0], s[1], s[2], s[3], s[4], count, 1.0 / count, m);
        out[p * 8 + ch] = pick(ch, m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7]);
        if (ch == 0u) out_passes[p] = c;
    }
}

__global__ __launch_bounds__(kBlock) void adaptive_count_kernel(uint32_t max_passes, uint64_t pixels, const uint32_t *__restrict__ passes,
                                                               uint32_t *__restrict__ reached) {
    uint32_t n = 0;
    for (uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x; p < pixels; p += (uint64_t)gridDim.x * kBlock)
        n += passes[p] == max_passes ? 1u : 0u;
    for (int off = 32; off > 0; off >>= 1) n += (uint32_t)__shfl_down((int)n, off);
    if ((threadIdx.x & 63u) == 0u && n != 0u) atomicAdd(reached, n);
}

}  // namespace adaptive

hipError_t launch_adaptive_select(const AdaptiveRule &rule, uint32_t rows, uint32_t width, const double *sums, const uint32_t *passes,
                                  unsigned char *hot, uint32_t *list, uint32_t *count, hipStream_t stream) {
    const uint64_t pixels = (uint64_t)rows * width;
    if (pixels == 0) return hipSuccess;
    if (pixels > 0x7fffffffull || rule.dilate > 2u) return hipErrorInvalidValue;
    const dim3 g((unsigned)((pixels + adaptive::kBlock - 1) / adaptive::kBlock)), b(adaptive::kBlock);
    hipError_t e = hipMemsetAsync(count, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    adaptive::adaptive_hot_kernel<<<g, b, 0, stream>>>(rule, pixels, sums, passes, hot);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    adaptive::adaptive_select_kernel<<<dim3((unsigned)((pixels + adaptive::kSelectBlock - 1) / adaptive::kSelectBlock)),
                                       dim3(adaptive::kSelectBlock), 0, stream>>>(rows, width, (int)rule.dilate, hot, list, count);
    return hipGetLastError();
}

hipError_t launch_adaptive_finish(uint32_t nsamp, uint64_t pixels, const double *sums, const uint32_t *passes, double *out_moments,
                                  uint32_t *out_passes, hipStream_t stream) {
    if (pixels == 0) return hipSuccess;
    if (pixels > 0x7fffffffull) return hipErrorInvalidValue;
    const uint64_t threads = pixels * 8;
    adaptive::adaptive_finish_kernel<<<dim3((unsigned)((threads + adaptive::kBlock - 1) / adaptive::kBlock)), dim3(adaptive::kBlock), 0,
                                       stream>>>(nsamp, pixels, sums, passes, out_moments, out_passes);
    return hipGetLastError();
}

hipError_t launch_adaptive_count(uint32_t max_passes, uint64_t pixels, const uint32_t *passes, uint32_t *reached, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(reached, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess || pixels == 0) return e;
    const uint64_t blocks = (pixels + adaptive::kBlock - 1) / adaptive::kBlock;
    adaptive::adaptive_count_kernel<<<dim3((unsigned)(blocks < 64 ? blocks : 64)), dim3(adaptive::kBlock), 0, stream>>>(max_passes, pixels,
                                                                                                                         passes, reached);
    return hipGetLastError();
}

}  // namespace flux
