// aov_chain_body.inc -- the feature buffers at the first NON-SPECULAR hit (include/flux_abi.h flux_render_aov_chain_rows*, DESIGN.md
// section 5i): aov_kernel's eight channels, taken where a sample's chain of delta bounces -- Reflective, Dielectric -- ends instead of
// where its primary ray lands, so that what a mirror or a pane of glass shows has edges in the denoisers' guides.  Included by
// render.hip behind moments_body.inc in ALL THREE copies, for moments_body.inc's reason: a Dielectric bounce runs dielectric_dir, so
// a scene with one needs the copy with the dielectric lobe; launch_plan.cpp plan_pass picks the copy as it does for the moments.
// Everything a sample runs is render_body.inc's or aov_body.inc's: primary_ray, path_begin, scene_hit with path_self, shade_hit for
// the bounce itself -- the child ray, the STRICT (f, s) stack entry and the FAST throughput are the render's bits, with no second
// copy of the lobe arithmetic here --, first_hit_fields for the fields of the hit the chain ends at, fold_path for the throughput.
//
// What a sample contributes, with K = max_chain the chain limit (1 <= K <= max_trace_depth, resolved by the caller):
//   segment k hits a Reflective or a Dielectric and k < K   the render's bounce; tsum += t; the next segment
//   a miss                                                  albedo fold(background), nothing else
//   any other hit (a delta material at k == K included)     albedo fold(a(m)), the hit's shading normal, depth tsum + t, a count of one
// fold(x) is fold_path on x in place of the path's end radiance.  With K = 1 no bounce runs, fold is the identity (x * 1.0 in FAST,
// no stack entry in STRICT) and tsum + t is 0.0 + t: the kernel writes aov_kernel's bits.  Values are not clamped.

// the material kind of the hit scene_hit<false, TRIS> reported (`hit` >= 0), from where first_hit_fields reads it
template <bool TRIS>
__device__ __forceinline__ int hit_material_kind(const RenderParams &P, int hit, int slot) {
    const bool is_tri = TRIS && slot >= 0;
#if FLUX_FAST
    if (is_tri) return P.mats[P.tris[slot].mat].kind;
    return reinterpret_cast<const DevHitRec *>(reinterpret_cast<const char *>(P.frec) + (uint32_t)hit * (uint32_t)sizeof(DevHitRec))->mat_kind;
#else
    return P.mats[is_tri ? P.tris[slot].mat : hit].kind;
#endif
}

// moments_kernel's layout (lane_group, pixels in row-major order), launch bounds and LDS: the STRICT (f, s) stack, the BVH stack behind
// it (bvh_stack_base).  The chain loop is per lane: a lane whose chain has ended waits for the longest chain of its wave.  The eight
// per-lane sums are combined by group_totals and the pixel's 64 bytes written as aov_kernel writes them.  No atomics, no statistics.
// P.out: [num_rows][W][FLUX_AOV_CHANNELS].
template <bool TRIS>
__global__ __launch_bounds__(FLUX_BLOCK_THREADS, FLUX_WPE_WIDE) void aov_chain_kernel(const RenderParams P, const int max_chain) {
    extern __shared__ double lds_stack[];
    const int tid = threadIdx.x;
    const int stride = blockDim.x;
    double *stk = lds_stack + tid;
    int *tstack = bvh_stack_base(lds_stack, P, stride) + tid;

    const uint32_t N = P.nsamp;
    const LaneGroup G = lane_group(N);
    const uint64_t pixel = G.unit();
    const bool lane_on = G.on((uint64_t)P.num_rows * P.img_w);
    int row = 0, col = 0;
    uint32_t set = 0;
    if (lane_on) {
        const uint64_t lrow = pixel / P.img_w;
        col = (int)(pixel - lrow * P.img_w);
        row = P.first_row + (int)lrow * P.row_stride;
        set = (uint32_t)P.rowperm[(size_t)row * P.num_sets + col] % P.num_sets;  // trace.rs:68-69
    }
    Stats st = {};
    double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // albedo, normal, t, hits
    const uint32_t nchunks = (N + 63u) / 64u;
    for (uint32_t c = 0; c < nchunks; ++c) {
        const uint32_t i = G.i0 + c * 64u;
        if (lane_on && i < N) {
            Path p;
            p.sq = P.pix[(size_t)set * N + i];
            const double2 lens = P.disc[(size_t)set * N + i];
            p.r = primary_ray(P, row, col, p.sq, lens);
            path_begin(p);
            double tsum = 0.0, t = 0.0;
            int hit, hslot;
            for (;;) {
                hslot = -1;
                hit = scene_hit<false, TRIS>(P, p.r, path_self(p), t, hslot, tstack, stride, st);
                if (hit < 0) break;  // scene.rs:168
                const int kind = hit_material_kind<TRIS>(P, hit, hslot);
                if ((kind != kMatReflective && kind != kMatDielectric) || p.depth >= max_chain) break;
                double Lr, Lg, Lb;  // (a delta material always bounces: shade_hit leaves them alone)
                shade_hit<false, TRIS>(P, p, set, i, hit, hslot, t, stk, stride, Lr, Lg, Lb, st);
                tsum += t;
            }
            double ar = P.bgr, ag = P.bgg, ab = P.bgb;
            if (hit >= 0) {
                V3 n, a;
                first_hit_fields<TRIS>(P, p.r, hit, hslot, t, n, a);  // (the emissive facing test with this segment's direction)
                ar = a.x;
                ag = a.y;
                ab = a.z;
                s[3] += n.x;
                s[4] += n.y;
                s[5] += n.z;
                s[6] += tsum + t;
                s[7] += 1.0;
            }
            fold_path(p, stk, stride, ar, ag, ab);
            s[0] += ar;
            s[1] += ag;
            s[2] += ab;
        }
    }
    double tot[8];
    group_totals<8>(G, s, tot);
    if (lane_on) {
        const double count = (double)N;
        double *o = P.out + pixel * 8;
        for (uint32_t ch = G.i0; ch < 8u; ch += G.lpp) {
            // (aov_kernel's select, a loop over the array, and its two means)
            double v = tot[0];
#pragma unroll
            for (int k = 1; k < 8; ++k) v = ch == (uint32_t)k ? tot[k] : v;
            if (ch == 6u) v = tot[7] > 0.0 ? v / tot[7] : 0.0;
            else v = v / count;
            o[ch] = v;
        }
    }
}
