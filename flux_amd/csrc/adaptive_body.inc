// adaptive_body.inc -- one pass of the adaptive sampler (include/flux_abi.h flux_render_adaptive_rows*, DESIGN.md section 5h): for
// every pixel of a work list, one more sample set of N samples, its five sums added to the pixel's running sums.  Included by
// render.hip behind moments_body.inc in ALL THREE copies, for moments_body.inc's reason: it runs the lobe code.  The sample loop and
// the combine are moments_kernel's own (trace_pixel_sums, moments_body.inc): a pass of a pixel that has taken none (c = 0) forms bit
// for bit the totals moments_kernel forms for it.  What decides which pixels a pass covers, and what turns the sums into the moments
// layout, holds no lobe code and lives in adaptive.hip.

// The pixel grid is replaced by a work list (AdaptiveWork, flux_device.h): entry e of the list names the pixel, local to the call,
// and the entries are the units of the layout (lane_group, render_body.inc), so a pass over a few per cent of the frame still runs
// on full waves.  Lanes past the list's end are idle.  A null list is the identity (the rounds in which every pixel is active), and in the call's first pass (AdaptiveWork::fresh) the state is
// taken as zero and overwritten, so the host clears nothing.  The pixel's pass count c picks the sample set,
// (set0 + c) mod S with set0 the set rowperm gives the pixel.  moments_kernel's launch bounds and LDS (launch_plan.cpp plan_pass).
// A pixel stands in a list at most once, so its state is read and written by one lane group alone: plain vector loads and stores,
// no atomics, no statistics.
template <bool TRIS>
__global__ __launch_bounds__(FLUX_BLOCK_THREADS, FLUX_WPE_WIDE) void adaptive_pass_kernel(const RenderParams P, const AdaptiveWork A) {
    extern __shared__ double lds_stack[];
    const int tid = threadIdx.x;
    const int stride = blockDim.x;
    double *stk = lds_stack + tid;
    int *tstack = bvh_stack_base(lds_stack, P, stride) + tid;

    const LaneGroup G = lane_group(P.nsamp);
    const bool lane_on = G.on((uint64_t)A.count);
    uint32_t pixel = 0, set = 0;
    if (lane_on) {
        pixel = A.list ? A.list[G.unit()] : (uint32_t)G.unit();
        const uint32_t lrow = pixel / (uint32_t)P.img_w;
        const uint32_t col = pixel - lrow * (uint32_t)P.img_w;
        const int row = P.first_row + (int)lrow * P.row_stride;
        const uint32_t set0 = (uint32_t)P.rowperm[(size_t)row * P.num_sets + col] % P.num_sets;  // trace.rs:68-69
        set = (set0 + (A.fresh ? 0u : A.passes[pixel])) % P.num_sets;
    }
    double tot[5];
    trace_pixel_sums<TRIS>(P, G, lane_on, pixel, set, stk, stride, tstack, tot);
    if (lane_on) {
        // one addition per running sum (pick's store order; lpp >= 4); lane 0 counts the pass
        double *o = A.sums + (size_t)pixel * kAdaptiveSums;
        for (uint32_t ch = G.i0; ch < (uint32_t)kAdaptiveSums; ch += G.lpp) o[ch] = (A.fresh ? 0.0 : o[ch]) + pick(ch, tot[0], tot[1], tot[2], tot[3], tot[4]);
        if (G.i0 == 0u) A.passes[pixel] = (A.fresh ? 0u : A.passes[pixel]) + 1u;
    }
}
