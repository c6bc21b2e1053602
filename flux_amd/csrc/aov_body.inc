// aov_body.inc -- the first-hit feature buffers (include/flux_abi.h flux_render_aov_rows*, DESIGN.md section 5e): per pixel the mean
// albedo, the mean shading normal, the mean hit distance and the coverage of the N primary rays the render kernels trace for it.
// Included by render.hip behind render_body.inc in the STRICT and the FAST copy (not the one with the dielectric lobe: a first hit
// runs no lobe, so a scene with a Dielectric uses the FAST copy); everything it calls -- primary_ray, scene_hit, map_wave,
// lane_group, group_totals -- is render_body.inc's, so a sample's ray, its first hit and its normal are the ones the render kernels and flux_debug_shade compute.
//
// What a sample contributes (shade_hit's fields of the hit, nothing of its bounce):
//   normal  the shading normal as the bounce would use it: a sphere's ((o - c) + t d) invert / radius, a plane's, disk's or triangle's
//           as stored, a box face's axis (negated for `invert`); a miss contributes 0;
//   albedo  the material's bounce weight in its closed form -- kd colour for Matte, ks colour for Reflective / Glossy, transmit_color
//           for a Dielectric: the records behind RenderParams::mats, which are a hit record's (fr, fg, fb) too --, for an Emissive
//           power colour on the side it emits to (materials.rs:44) and 0 on the other; on a triangle with vertex colours (DESIGN.md
//           section 5k) times the interpolated colour factor; a miss contributes the background;
//   t, 1    the hit distance and a count of one; a miss contributes neither.
// Values are not clamped.

// the closed-form bounce weight of material `mat` (scene_build.cpp: 32 B a record behind the n_mats materials)
constexpr uint32_t kMaterialWeightBytes = 32;
__device__ __forceinline__ const char *material_weights(const RenderParams &P) { return reinterpret_cast<const char *>(P.mats + P.n_mats); }
__device__ __forceinline__ V3 material_weight(const RenderParams &P, int mat) {
    const double *w = reinterpret_cast<const double *>(material_weights(P)) + 4 * (size_t)mat;
    return mk(w[0], w[1], w[2]);
}

// Normal and albedo of the hit scene_hit<false, TRIS> reported for ray r (`hit` >= 0): the fields as shade_hit takes them -- from
// DevHitRec / DevTri + the material in FAST, from DevShape with the box's face in the slot (-2 - face) in STRICT
template <bool TRIS>
__device__ __forceinline__ void first_hit_fields(const RenderParams &P, const Ray &r, int hit, int slot, double t, V3 &n, V3 &a) {
    const bool is_tri = TRIS && slot >= 0;
    const V3 d = mk(r.dx, r.dy, r.dz);
    int kind;
#if FLUX_FAST
    // (the two sources meet in six scalars: joined as two V3 written through the references, the compiler kept them in scratch)
    double nx, ny, nz, wr, wg, wb;
    if (is_tri) {
        const DevTri &T = P.tris[slot];
        const int mat = T.mat;
        const V3 tn = tri_shading_normal(P, r, slot, material_weights(P), kMaterialWeightBytes, mat, wr, wg, wb);  // (vertex colours: §5k)
        nx = tn.x; ny = tn.y; nz = tn.z;
        kind = P.mats[mat].kind;
    } else {
        const DevHitRec &R = *reinterpret_cast<const DevHitRec *>(reinterpret_cast<const char *>(P.frec) + (uint32_t)hit * (uint32_t)sizeof(DevHitRec));
        kind = R.mat_kind;
        wr = R.fr; wg = R.fg; wb = R.fb;
        // sphere: (temp + t d) * invert_val / radius with invert_val/radius in one rounding; plane, disk, box face: stored normal
        const V3 ns = mk(((r.ox - R.cx) + t * d.x) * R.inv_rad, ((r.oy - R.cy) + t * d.y) * R.inv_rad, ((r.oz - R.cz) + t * d.z) * R.inv_rad);
        const bool sph = R.shape_kind == kShapeSphere;
        nx = sph ? ns.x : R.cx; ny = sph ? ns.y : R.cy; nz = sph ? ns.z : R.cz;
    }
    n = mk(nx, ny, nz);
    a = mk(wr, wg, wb);
#else
    const DevShape *S = P.shapes + (is_tri ? 0 : hit);
    const int mat = is_tri ? P.tris[slot].mat : hit;
    double wr = 0.0, wg = 0.0, wb = 0.0;  // a triangle's weight, times its colour factor where it has one (DESIGN.md section 5k)
    if (is_tri) {
        n = tri_shading_normal(P, r, slot, material_weights(P), kMaterialWeightBytes, mat, wr, wg, wb);
    } else if (S->kind == kShapeSphere) {
        const double inv = S->inv, rad = S->radius;
        n = mk(((r.ox - S->px) + t * d.x) * inv / rad, ((r.oy - S->py) + t * d.y) * inv / rad, ((r.oz - S->pz) + t * d.z) * inv / rad);
    } else if (S->kind == kShapeBox) {
        const int face = -2 - slot;
        const double v = ((face & 1) ? 1.0 : -1.0) * S->inv;
        n = mk(face < 2 ? v : 0.0, (face >> 1) == 1 ? v : 0.0, face >= 4 ? v : 0.0);
    } else {
        n = mk(S->c0x, S->c0y, S->c0z);
    }
    kind = P.mats[mat].kind;
    // (three scalars, joined here: written through `a` in the branch, the compiler kept the triple in scratch)
    a = is_tri ? mk(wr, wg, wb) : material_weight(P, mat);
#endif
    if (kind == kMatEmissive) {  // materials.rs:41-50: black from behind
        const bool front = ((n.x * -1.0) * d.x + (n.y * -1.0) * d.y + (n.z * -1.0) * d.z) > 0.0;
        a = mk(front ? a.x : 0.0, front ? a.y : 0.0, front ? a.z : 0.0);
    }
}

// One wave per pixel from 64 samples on (lane l takes samples l, l + 64, ...; pixels in map_wave's order, so a set's tables stay in
// one XCD's L2), lane_group's groups in row-major order below (render_body.inc).  The eight per-lane sums are combined by
// group_totals and the pixel's 64 bytes written as one line, a double per lane.  No atomics, no statistics.
// P.out: [num_rows][W][FLUX_AOV_CHANNELS].  Dynamic LDS: the per-lane BVH stack [entry][thread] of a mesh scene, at the
// base in both copies (no recursion stack in front of it here, unlike bvh_stack_base's STRICT layout): launch_plan.cpp plan_pass.
template <bool TRIS>
__global__ __launch_bounds__(FLUX_BLOCK_THREADS, FLUX_WPE_WIDE) void aov_kernel(const RenderParams P) {
    extern __shared__ double lds_stack[];
    const int tid = threadIdx.x;
    const int stride = blockDim.x;
    int *tstack = reinterpret_cast<int *>(lds_stack) + tid;

    const uint32_t N = P.nsamp;
    const LaneGroup G = lane_group(N);
    int row = 0, col = 0;
    uint32_t set = 0;
    uint64_t pixel = 0;
    bool lane_on;
    if (G.whole_wave) {
        int lrow;
        lane_on = map_wave(P, G.wave, lrow, col, row, set, pixel);
    } else {
        pixel = G.unit();
        lane_on = G.on((uint64_t)P.num_rows * P.img_w);
        if (lane_on) {
            const uint64_t lrow = pixel / P.img_w;
            col = (int)(pixel - lrow * P.img_w);
            row = P.first_row + (int)lrow * P.row_stride;
            set = (uint32_t)P.rowperm[(size_t)row * P.num_sets + col] % P.num_sets;  // trace.rs:68-69
        }
    }
    Stats st = {};
    double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // albedo, normal, t, hits
    const uint32_t nchunks = (N + 63u) / 64u;
    for (uint32_t c = 0; c < nchunks; ++c) {
        const uint32_t i = G.i0 + c * 64u;
        if (lane_on && i < N) {
            const double2 sq = P.pix[(size_t)set * N + i];
            const double2 lens = P.disc[(size_t)set * N + i];
            const Ray r = primary_ray(P, row, col, sq, lens);
            double t = 0.0;
            int hslot = -1;
            const int hit = scene_hit<false, TRIS>(P, r, -1, t, hslot, tstack, stride, st);
            if (hit < 0) {  // scene.rs:168
                s[0] += P.bgr;
                s[1] += P.bgg;
                s[2] += P.bgb;
            } else {
                V3 n, a;
                first_hit_fields<TRIS>(P, r, hit, hslot, t, n, a);
                s[0] += a.x;
                s[1] += a.y;
                s[2] += a.z;
                s[3] += n.x;
                s[4] += n.y;
                s[5] += n.z;
                s[6] += t;
                s[7] += 1.0;
            }
        }
    }
    double tot[8];
    group_totals<8>(G, s, tot);
    if (lane_on) {
        const double count = (double)N;
        double *o = P.out + pixel * 8;
        for (uint32_t ch = G.i0; ch < 8u; ch += G.lpp) {
            // (the select as a loop over the array, not pick's chain over values: the compiler keeps this kernel's eight totals in
            // scratch and indexes them, and with the chain it spilled 55 SGPRs for 23 and ran 6 to 9 % longer on demo2)
            double v = tot[0];
#pragma unroll
            for (int k = 1; k < 8; ++k) v = ch == (uint32_t)k ? tot[k] : v;
            // depth: the mean over the samples that hit (0 where none did; a plane's +inf passes through); every other channel: over all N
            if (ch == 6u) v = tot[7] > 0.0 ? v / tot[7] : 0.0;
            else v = v / count;
            o[ch] = v;
        }
    }
}
