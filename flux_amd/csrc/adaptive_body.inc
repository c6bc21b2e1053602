// adaptive_body.inc -- one pass of the adaptive sampler (include/flux_abi.h flux_render_adaptive_rows*, DESIGN.md section 5h): for
// every pixel of a work list, one more sample set of N samples, its five sums added to the pixel's running sums.  Included by
// render.hip behind moments_body.inc in ALL THREE copies, for moments_body.inc's reason: it runs the lobe code.  Everything a sample
// runs -- primary_ray, path_begin, shade_level, fold_path -- is render_body.inc's, in moments_kernel's order, and the five per-lane
// sums are combined as moments_kernel combines them: a pass of a pixel that has taken none (c = 0) forms bit for bit the totals
// moments_kernel forms for it.  What decides which pixels a pass covers, and what turns the sums into the moments layout, holds no
// lobe code and lives in adaptive.hip.

// The pixel grid is replaced by a work list (AdaptiveWork, flux_device.h): entry e of the list names the pixel, local to the call.
// From 64 samples on a wave takes one entry (lane l takes samples l, l + 64, ...); below, 64 / N consecutive entries share a wave
// in lane groups, so a pass over a few per cent of the frame still runs on full waves.  Lanes past the list's end are idle.  A null
// list is the identity (the rounds in which every pixel is active), and in the call's first pass (AdaptiveWork::fresh) the state is
// taken as zero and overwritten, so the host clears nothing.  The pixel's pass count c picks the sample set,
// (set0 + c) mod S with set0 the set rowperm gives the pixel.  moments_kernel's launch bounds and LDS (the STRICT (f, s) stack, the
// BVH stack behind it: launch_plan.cpp plan_adaptive).  A pixel stands in a list at most once, so its state is read and written by
// one lane group alone: plain vector loads and stores, no atomics, no statistics.
template <bool TRIS>
__global__ __launch_bounds__(FLUX_BLOCK_THREADS, FLUX_WPE_WIDE) void adaptive_pass_kernel(const RenderParams P, const AdaptiveWork A) {
    extern __shared__ double lds_stack[];
    const int tid = threadIdx.x;
    const uint32_t lane = tid & 63;
    const int stride = blockDim.x;
    double *stk = lds_stack + tid;
    int *tstack = bvh_stack_base(lds_stack, P, stride) + tid;

    const uint32_t N = P.nsamp;
    const uint32_t lpp = N >= 64u ? 64u : N;  // lanes per pixel
    const uint32_t ppw = 64u / lpp;           // list entries per wave
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (tid >> 6);
    const uint32_t slot = lane / lpp;
    const uint32_t seg_base = slot * lpp;
    const uint32_t i0 = lane - seg_base;
    const uint64_t entry = wave * ppw + slot;
    const bool lane_on = slot < ppw && entry < (uint64_t)A.count;

    uint32_t pixel = 0, set = 0;
    if (lane_on) {
        pixel = A.list ? A.list[entry] : (uint32_t)entry;
        const uint32_t lrow = pixel / (uint32_t)P.img_w;
        const uint32_t col = pixel - lrow * (uint32_t)P.img_w;
        const int row = P.first_row + (int)lrow * P.row_stride;
        const uint32_t set0 = (uint32_t)P.rowperm[(size_t)row * P.num_sets + col] % P.num_sets;  // trace.rs:68-69
        set = (set0 + (A.fresh ? 0u : A.passes[pixel])) % P.num_sets;
    }
    Stats st = {};
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};  // r, g, b, l, l l
    const uint32_t nchunks = (N + 63u) / 64u;
    for (uint32_t c = 0; c < nchunks; ++c) {
        const uint32_t i = i0 + c * 64u;
        if (lane_on && i < N) {
            // (row and col formed again per chunk from a copy of `pixel` the compiler cannot see through: moments_kernel's measure
            // against the spill of the mesh instantiations, moments_body.inc)
            uint32_t px = pixel;
            asm("" : "+v"(px));
            const uint32_t lrow = px / (uint32_t)P.img_w;
            const int col = (int)(px - lrow * (uint32_t)P.img_w);
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
    if (lpp == 64u) {  // wave-uniform: the whole wave is one entry
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
        // lane j of the entry's group adds sums j, j + lpp, ... (lpp >= 4): one addition per running sum; lane 0 counts the pass
        double *o = A.sums + (size_t)pixel * kAdaptiveSums;
        for (uint32_t ch = i0; ch < (uint32_t)kAdaptiveSums; ch += lpp) {
            double v = tot[0];
            v = ch == 1u ? tot[1] : v;
            v = ch == 2u ? tot[2] : v;
            v = ch == 3u ? tot[3] : v;
            v = ch == 4u ? tot[4] : v;
            o[ch] = (A.fresh ? 0.0 : o[ch]) + v;
        }
        if (i0 == 0u) A.passes[pixel] = (A.fresh ? 0u : A.passes[pixel]) + 1u;
    }
}

static hipError_t launch_adaptive_impl(const LaunchPlan &L, const RenderParams &p, const AdaptiveWork &a, hipStream_t stream) {
    if (L.blocks > 0x7fffffffull) return hipErrorInvalidValue;
    const dim3 g((unsigned)L.blocks), b(L.block);
    if (L.tris) adaptive_pass_kernel<true><<<g, b, L.lds, stream>>>(p, a);
    else adaptive_pass_kernel<false><<<g, b, L.lds, stream>>>(p, a);
    return hipGetLastError();
}
