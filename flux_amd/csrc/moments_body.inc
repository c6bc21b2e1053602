// moments_body.inc -- the per-pixel sample moments (include/flux_abi.h flux_render_moments_rows*, DESIGN.md section 5g): per pixel the
// frame as flux_render_rows gives it, the unclamped mean radiance, the sample variance of the luminance and the variance of the
// frame's luminance estimate.  Included by render.hip behind render_body.inc (and aov_body.inc) in ALL THREE copies -- it runs the lobe
// code, so a scene with a Dielectric needs the copy with the dielectric lobe; launch_plan.cpp plan_moments picks the copy as
// plan_render does.  Everything a sample runs -- primary_ray, path_begin, shade_level, fold_path -- is render_body.inc's, in
// render_static_kernel's order: a sample's radiance is bit for bit the one that kernel adds up.
//
// Per sample, with L the folded radiance and l = (0.2126 L.r + 0.7152 L.g) + 0.0722 L.b, a lane accumulates the five sums
// r, g, b, l and l l: the one-pass form.  At preview sample counts it agrees with the two-pass variance to rounding level
// (section 5g has the bound, about N 2^-53 (1 + m^2 / s^2) relative).  With N the sample count:
//   mean  = sum c * pixel_denom                                             channels 4-6 (FLUX_MOMENT_MEAN), unclamped
//   rgb   = max_to_one(mean), finish_pixel's operations in its order         channels 0-2 (FLUX_MOMENT_RGB)
//   s2    = max(0, sum l^2 - (sum l * sum l) / N) / (N - 1)                  channel 7 (FLUX_MOMENT_S2); the max keeps a NaN
//   var   = (s2 / N) * (k * k), k = 1 / max(mean) where that exceeds 1       channel 3 (FLUX_MOMENT_VAR): the variance of lum(rgb)
// Nothing else is clamped: a NaN or inf sample shows in channels 3 and 7.

// One wave per pixel from 64 samples on (lane l takes samples l, l + 64, ...), 64 / N pixels per wave in lane groups below:
// render_static_kernel's two layouts, its launch bounds and its LDS (the STRICT (f, s) stack, the BVH stack behind it).  The five
// per-lane sums are combined as finish_pixel combines three -- wave_sum1's tree, or lane order within a group --, so the buffer is
// bit-reproducible and does not depend on how rows are grouped into calls; the pixel's 64 bytes are then written as one line, a
// double per lane (aov_kernel's store).  No atomics, no statistics.  P.out: [num_rows][W][FLUX_MOMENT_CHANNELS].
template <bool TRIS>
__global__ __launch_bounds__(FLUX_BLOCK_THREADS, FLUX_WPE_WIDE) void moments_kernel(const RenderParams P) {
    extern __shared__ double lds_stack[];
    const int tid = threadIdx.x;
    const uint32_t lane = tid & 63;
    const int stride = blockDim.x;
    double *stk = lds_stack + tid;
    int *tstack = bvh_stack_base(lds_stack, P, stride) + tid;

    const uint32_t N = P.nsamp;
    const uint32_t lpp = N >= 64u ? 64u : N;  // lanes per pixel
    const uint32_t ppw = 64u / lpp;           // pixels per wave
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (tid >> 6);
    const uint32_t slot = lane / lpp;
    const uint32_t seg_base = slot * lpp;
    const uint32_t i0 = lane - seg_base;
    const uint64_t npix = (uint64_t)P.num_rows * P.img_w;
    const uint64_t pixel = wave * ppw + slot;
    const bool lane_on = slot < ppw && pixel < npix;

    uint32_t set = 0;
    if (lane_on) {
        const uint64_t lrow = pixel / P.img_w;
        const int col = (int)(pixel - lrow * P.img_w);
        const int row = P.first_row + (int)lrow * P.row_stride;
        set = (uint32_t)P.rowperm[(size_t)row * P.num_sets + col] % P.num_sets;  // trace.rs:68-69
    }
    Stats st = {};
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};  // r, g, b, l, l l
    const uint32_t nchunks = (N + 63u) / 64u;
    for (uint32_t c = 0; c < nchunks; ++c) {
        const uint32_t i = i0 + c * 64u;
        if (lane_on && i < N) {
            // row and col are formed again per chunk, from a copy of `pixel` the compiler cannot see through: the two sums this kernel
            // carries beyond render_static_kernel's three are four VGPRs live across the path loop, and with row and col live there
            // too the mesh instantiations of the FAST copies spilled 4 VGPRs.  (A 32-bit division in its place measured the same:
            // the division is not what the pass costs beyond the static kernel, DESIGN.md section 5g.)
            uint64_t px = pixel;
            asm("" : "+v"(px));  // (not volatile: that would count as a store, and no record after it could be a scalar load)
            const uint64_t lrow = px / P.img_w;
            const uint32_t pcol = (uint32_t)(px - lrow * P.img_w);
            const int col = (int)pcol;
            const int row = P.first_row + (int)lrow * P.row_stride;
            Path p;
            p.sq = P.pix[(size_t)set * N + i];
            const double2 lens = P.disc[(size_t)set * N + i];
            p.r = primary_ray(P, row, col, p.sq, lens);
            path_begin(p);
            double Lr, Lg, Lb;
            while (shade_level<false, TRIS>(P, p, set, i, stk, stride, tstack, Lr, Lg, Lb, st)) {
            }
            fold_path(p, stk, stride, Lr, Lg, Lb);
            const double l = (0.2126 * Lr + 0.7152 * Lg) + 0.0722 * Lb;
            s[0] += Lr;  // trace.rs:82
            s[1] += Lg;
            s[2] += Lb;
            s[3] += l;
            s[4] += l * l;
        }
    }
    double tot[5];
    if (lpp == 64u) {  // wave-uniform: the whole wave is one pixel
#pragma unroll
        for (int k = 0; k < 5; ++k) tot[k] = wave_sum1(s[k]);
    } else {
#pragma unroll
        for (int k = 0; k < 5; ++k) tot[k] = 0.0;
        for (uint32_t j = 0; j < lpp; ++j) {
            const int src = (int)((seg_base + j) & 63u);
#pragma unroll
            for (int k = 0; k < 5; ++k) tot[k] += __shfl(s[k], src);
        }
    }
    if (lane_on) {
        // finish_pixel: * 1/n^2, then Color::max_to_one (color.rs:35-44)
        const double mr = tot[0] * P.pixel_denom, mg = tot[1] * P.pixel_denom, mb = tot[2] * P.pixel_denom;
        double r = mr, g = mg, b = mb, k = 1.0;
        const double mx1 = r > g ? r : g;
        const double mx2 = mx1 > b ? mx1 : b;
        if (mx2 > 1.0) {
            k = 1.0 / mx2;
            r *= k;
            g *= k;
            b *= k;
        }
        const double count = (double)N;
        const double d = tot[4] - (tot[3] * tot[3]) / count;
        const double s2 = (d < 0.0 ? 0.0 : d) / (count - 1.0);  // (a NaN stays a NaN)
        const double var = (s2 / count) * (k * k);
        // lane j of the pixel's group writes channels j, j + lpp, ...: from 8 samples on, lanes 0..7 one double each
        double *o = P.out + pixel * 8;
        for (uint32_t ch = i0; ch < 8u; ch += lpp) {
            double v = r;
            v = ch == 1u ? g : v;
            v = ch == 2u ? b : v;
            v = ch == 3u ? var : v;
            v = ch == 4u ? mr : v;
            v = ch == 5u ? mg : v;
            v = ch == 6u ? mb : v;
            v = ch == 7u ? s2 : v;
            o[ch] = v;
        }
    }
}

static hipError_t launch_moments_impl(const LaunchPlan &L, const RenderParams &p, hipStream_t stream) {
    if (L.blocks > 0x7fffffffull) return hipErrorInvalidValue;
    const dim3 g((unsigned)L.blocks), b(L.block);
    if (L.tris) moments_kernel<true><<<g, b, L.lds, stream>>>(p);
    else moments_kernel<false><<<g, b, L.lds, stream>>>(p);
    return hipGetLastError();
}
