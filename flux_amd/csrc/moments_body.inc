// moments_body.inc -- the per-pixel sample moments (include/flux_abi.h flux_render_moments_rows*, DESIGN.md section 5g): per pixel the
// frame as flux_render_rows gives it, the unclamped mean radiance, the sample variance of the luminance and the variance of the
// frame's luminance estimate.  Included by render.hip behind render_body.inc (and aov_body.inc) in ALL THREE copies -- it runs the lobe
// code, so a scene with a Dielectric needs the copy with the dielectric lobe; launch_plan.cpp plan_pass picks the copy as
// plan_render does.  Everything a sample runs -- primary_ray, path_begin, shade_level, fold_path -- is render_body.inc's, in
// render_static_kernel's order: a sample's radiance is bit for bit the one that kernel adds up.
//
// Per sample, with L the folded radiance and l = (0.2126 L.r + 0.7152 L.g) + 0.0722 L.b, a lane accumulates the five sums
// r, g, b, l and l l: the one-pass form.  At preview sample counts it agrees with the two-pass variance to rounding level
// (section 5g has the bound, about N 2^-53 (1 + m^2 / s^2) relative).  What the sums become is moments_of_sums' (flux_moments.h).

// The sample loop of a pass that keeps those five sums, for moments_kernel (PIX = uint64_t) and adaptive_pass_kernel (adaptive_body.inc,
// PIX = uint32_t: the width of the division that splits `pixel`, local to the call, into row and column): the group's samples of sample
// set `set` traced for the pixel in render_static_kernel's order, then the five totals of the group (group_totals).  No statistics.
template <bool TRIS, class PIX>
__device__ __forceinline__ void trace_pixel_sums(const RenderParams &P, const LaneGroup &G, bool lane_on, PIX pixel, uint32_t set,
                                                 double *stk, int stride, int *tstack, double (&tot)[5]) {
    const uint32_t N = P.nsamp;
    Stats st = {};
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};  // r, g, b, l, l l
    const uint32_t nchunks = (N + 63u) / 64u;
    for (uint32_t c = 0; c < nchunks; ++c) {
        const uint32_t i = G.i0 + c * 64u;
        if (lane_on && i < N) {
            // row and col are formed per chunk, from a copy of `pixel` the compiler cannot see through: the two sums carried
            // beyond render_static_kernel's three are four VGPRs live across the path loop, and with row and col live there
            // too the mesh instantiations of the FAST copies spilled 4 VGPRs.  (A 32-bit division in the 64-bit one's place measured
            // the same: the division is not what the pass costs beyond the static kernel, DESIGN.md section 5g.)
            PIX px = pixel;
            asm("" : "+v"(px));  // (not volatile: that would count as a store, and no record after it could be a scalar load)
            const PIX lrow = px / (PIX)P.img_w;
            const int col = (int)(px - lrow * (PIX)P.img_w);
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
    group_totals<5>(G, s, tot);
}

// render_static_kernel's layout (lane_group), launch bounds and LDS (the STRICT (f, s) stack, the BVH stack behind it), pixels in
// row-major order.  The pixel's 64 bytes are written as one line (pick).  No atomics.  P.out: [num_rows][W][FLUX_MOMENT_CHANNELS].
template <bool TRIS>
__global__ __launch_bounds__(FLUX_BLOCK_THREADS, FLUX_WPE_WIDE) void moments_kernel(const RenderParams P) {
    extern __shared__ double lds_stack[];
    const int tid = threadIdx.x;
    const int stride = blockDim.x;
    double *stk = lds_stack + tid;
    int *tstack = bvh_stack_base(lds_stack, P, stride) + tid;

    const LaneGroup G = lane_group(P.nsamp);
    const uint64_t pixel = G.unit();
    const bool lane_on = G.on((uint64_t)P.num_rows * P.img_w);
    uint32_t set = 0;
    if (lane_on) {
        const uint64_t lrow = pixel / P.img_w;
        const int col = (int)(pixel - lrow * P.img_w);
        const int row = P.first_row + (int)lrow * P.row_stride;
        set = (uint32_t)P.rowperm[(size_t)row * P.num_sets + col] % P.num_sets;  // trace.rs:68-69
    }
    double tot[5];
    trace_pixel_sums<TRIS>(P, G, lane_on, pixel, set, stk, stride, tstack, tot);
    if (lane_on) {
        double m[8];
        moments_of_sums(tot[0], tot[1], tot[2], tot[3], tot[4], (double)P.nsamp, P.pixel_denom, m);
        double *o = P.out + pixel * 8;
        for (uint32_t ch = G.i0; ch < 8u; ch += G.lpp) o[ch] = pick(ch, m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7]);
    }
}
