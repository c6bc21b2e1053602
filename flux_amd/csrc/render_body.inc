// render_body.inc -- the per-pixel render loop, included TWICE by render.hip:
//   FLUX_FAST == 0  namespace flux::strict   `#pragma clang fp contract(off)`
//       the reference's operation order, IEEE division/sqrt, OCML pow/sincos, BoundingBox::hit before
//       every sphere, (f,s) recursion stack folded from the deepest bounce outward;
//   FLUX_FAST == 1  namespace flux::fast     `#pragma clang fp contract(fast)`
//       the same estimator, evaluated for the machine: FMA contraction, flux_math.h elementary
//       functions, no bounding-box pre-test (the quadratic implies its answer -- the sphere lies inside the box -- in every
//       case but one, which is reproduced explicitly: box_z_nan_miss),
//       path throughput kept in registers, and each bounce's weight f * (n.wi)/pdf taken in the closed
//       form the reference's long form reduces to (Matte: f/INV_PI; PerfectSpecular: f; Glossy: cs ks --
//       pdf = lobe (n.wi) and f = cs ks lobe, so the lobe and n.wi cancel; SURVEY.md 8(a) "hand-checkable
//       consequences").  The two agree to ~2 ulp wherever the reference's arithmetic is healthy; where the
//       long form breaks down (a Phong lobe that under/overflows -- needs a non-unit plane normal -- or
//       n.wi == 0) the reference returns NaN or a subnormal-degraded value and FAST the analytic one.
//       Still FP64 end to end; differs from strict by rounding.
// Both are checked against the CPU restatement at the north-star tolerance (tests/test_gpu_parity.py).
//
// Replaces Camera::render (fluxcore/src/trace.rs:53-97) and everything it calls: see render.hip.

// FAST: stage boundaries the instruction scheduler may not move code across.  Without them it
// interleaves the independent polynomial chains of sincos / pow / rsqrt for ILP, lengthening live ranges
// (measured neutral since the coefficients left the VGPRs; kept as documentation of the stage structure).
#undef FLUX_STAGE
#if FLUX_FAST
#define FLUX_STAGE() __builtin_amdgcn_sched_barrier(0)
#else
#define FLUX_STAGE() ((void)0)
#endif

struct Ray {
    double ox, oy, oz, dx, dy, dz;
};

typedef const __attribute__((address_space(4))) RenderParams *ParamsInKernarg;
// Kernel arguments re-read in every pass of a persistent loop.  Handed the plain by-value struct, the
// compiler loads every field a loop will ever need ONCE, before the loop, keeps well over a hundred scalar registers' worth
// alive across it and spills the excess into vector-register lanes -- a v_readlane (a VALU issue slot) per use, a v_writelane
// per update.  Read through this view instead, a field is loaded where the pass uses it (a scalar load from the kernarg
// segment, served by the scalar cache) and is dead again at the end of the pass.
// The view: the kernel's one by-value argument where it lives, at offset 0 of the kernarg segment (taking the parameter's
// address would make a private copy of the whole struct in scratch memory), passed through an empty asm so that it is a new
// value in every pass and no load can move above it.
// (`tick` is any wave-uniform value that changes from pass to pass: it keeps the -- deliberately NOT volatile, see trav_pin4 --
// asm inside the loop)
// ONLY for kernels whose FIRST (and by-value) argument is the RenderParams -- it reads the kernarg segment at offset 0; every
// kernel of this file is declared that way (`const RenderParams P0` and nothing in front of it), and one that is not must not
// call this.
static_assert(sizeof(DevMaterial) % 16 == 0, "the bounce-weight records behind the materials are read as double2");
__device__ __forceinline__ const RenderParams &relaunder_params(uint32_t tick) {
    ParamsInKernarg p = (ParamsInKernarg)__builtin_amdgcn_kernarg_segment_ptr();
    asm("" : "+s"(p) : "s"(tick));
    return *(const RenderParams *)p;
}

// The depth limit and the depth cut's depth as phase B takes them.  PAIR (split_depth_pair: the TYP instantiations of render_split_kernel):
// RenderParams::depth_pair, ONE 64-bit scalar load where phase B needs the limit, in front of its scan.  Two field reads are two loads to
// the compiler, and it places the cut's at its use, behind the scan and the shading step: a scalar load and its full wait between the
// classification and the park, in every pass.  It costs the TYP instantiations no register -- the headline stays at 84 vector and 96
// scalar registers, the others drop two scalar ones.  The instantiations without TYP stand at the scalar-register limit and spill to
// vector lanes as they are; one more value held across the scan is two to four more spills there, so they read the two fields where
// they use them, the parent's code (profiles/r16_plane_div/registers.txt).
struct SplitDepths {
    int max_depth, cut_depth;
};
constexpr bool split_depth_pair(bool TYP) { return TYP; }
template <bool PAIR>
__device__ __forceinline__ SplitDepths split_depths(const RenderParams &P) {
    if (!PAIR) return SplitDepths{0, 0};  // (not read: split_max_depth, split_cut_depth below)
    // (a typed 64-bit load: a byte copy is a load of alignment 1, which no scalar load serves -- it came out a vector load)
    typedef unsigned long long __attribute__((may_alias)) DepthPair;
    const DepthPair both = *reinterpret_cast<const DepthPair *>(P.depth_pair);
    return SplitDepths{(int)(uint32_t)both, (int)(uint32_t)(both >> 32)};
}
// (without PAIR: the field, read where the value is used)
template <bool PAIR>
__device__ __forceinline__ int split_max_depth(const RenderParams &P, const SplitDepths &d) { return PAIR ? d.max_depth : P.max_depth; }
template <bool PAIR>
__device__ __forceinline__ int split_cut_depth(const RenderParams &P, const SplitDepths &d) { return PAIR ? d.cut_depth : P.cut_depth; }

// wave votes straight from the compare's lane mask (hip's __ballot / __any / __all go through a 0/1 select and a second compare)
__device__ __forceinline__ unsigned long long ballot64(bool b) { return __builtin_amdgcn_ballot_w64(b); }
__device__ __forceinline__ bool any64(bool b) { return __builtin_amdgcn_ballot_w64(b) != 0ull; }
__device__ __forceinline__ bool all64(bool b) { return __builtin_amdgcn_ballot_w64(!b) == 0ull; }
// The active lanes whose d_a plane_div_admits (flux_plane_axis.h: its f32 image a normal number), as the votes of both scans take it:
// ONE class test that writes the lane mask (the bits of lanes that are not active are zero).  Written out because a ballot of
// __builtin_isnormal is the class test, a 0/1 select and a compare of that -- and its mask a vector register; the probe kernel
// holds this mask to the function lane by lane (render.hip plane_div_probe_kernel, tests/test_gpu_plane_div.py).
__device__ __forceinline__ unsigned long long plane_div_admits_lanes(double da) {
    unsigned long long m;
    asm("v_cmp_class_f32_e64 %0, %1, %2" : "=s"(m) : "v"((float)da), "s"(0x108));  // 0x108: -normal | +normal
    return m;
}

// A gather from a table in GLOBAL memory: wave-uniform base + 32-bit per-lane byte offset.  A base that comes out of a record in memory
// (DevSetRows) is a generic pointer to the compiler: flat_load with a 64-bit address per lane, formed by two or three VALU instructions
// per gather.  Told that it is global, it emits global_load with the scalar base and the 32-bit offset.
typedef double flux_d2 __attribute__((ext_vector_type(2)));
template <class T>
__device__ __forceinline__ T gather_global(const void *base, uint32_t byte_off) {
    typedef const __attribute__((address_space(1))) char *gchar;
    typedef const __attribute__((address_space(1))) T *gT;
    return *(gT)((gchar)base + byte_off);
}
__device__ __forceinline__ double2 gather_global_d2(const void *base, uint32_t byte_off) {
    const flux_d2 v = gather_global<flux_d2>(base, byte_off);
    return make_double2(v.x, v.y);
}

// A sample set's table rows (DevSetRows) by a 32-bit BYTE offset from the wave-uniform base: the scalar load takes it as its offset
// operand.  (As an index the compiler widened it: a 64-bit shift and a 64-bit add -- four scalar instructions -- at every use.)
__device__ __forceinline__ const DevSetRows &set_rows_of(const RenderParams &P, uint32_t set) {
    return *reinterpret_cast<const DevSetRows *>(reinterpret_cast<const char *>(P.set_rows) + (set << 6));
}

// -DFLUX_DEBUG_TRIPS (experiment builds, scripts/): wave-level trip counts of the loop sections, added by the first
// active lane to the statistics slots 10..15 (stats must be enabled) -- on top of the dielectric counters in 10 and 11, which
// such a build does not keep apart; never in the product build.
#ifndef FLUX_TRIP_DEFINED
#define FLUX_TRIP_DEFINED
#ifdef FLUX_DEBUG_TRIPS
#define FLUX_TRIP(P, slot)                                                                                   \
    do {                                                                                                     \
        const unsigned long long ex_ = ballot64(1);                                                          \
        if ((P).stats && __builtin_amdgcn_mbcnt_hi((uint32_t)(ex_ >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ex_, 0u)) == 0) \
            atomicAdd((P).stats + (slot), 1ull);                                                             \
    } while (0)
// the same with the number of active lanes added to the following slot
#define FLUX_TRIP_LANES(P, slot)                                                                             \
    do {                                                                                                     \
        const unsigned long long ex_ = ballot64(1);                                                          \
        if ((P).stats && __builtin_amdgcn_mbcnt_hi((uint32_t)(ex_ >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ex_, 0u)) == 0) { \
            atomicAdd((P).stats + (slot), 1ull);                                                             \
            atomicAdd((P).stats + (slot) + 1, (unsigned long long)__popcll(ex_));                            \
        }                                                                                                    \
    } while (0)
#else
#define FLUX_TRIP(P, slot) ((void)0)
#define FLUX_TRIP_LANES(P, slot) ((void)0)
#endif
#endif
// -DFLUX_DEBUG_SCENSUS (experiment builds, scripts/strict_census.py): STRICT's per-lane candidate loop -- (executions, active lanes) of
// the scan (slots 10, 11), of a candidate trip = one box test (12, 13) and of the quadratic behind it (14, 15)
#ifndef FLUX_SCENSUS_DEFINED
#define FLUX_SCENSUS_DEFINED
#ifdef FLUX_DEBUG_SCENSUS
#define FLUX_SCENSUS(P, slot)                                                                                \
    do {                                                                                                     \
        const unsigned long long ex_ = ballot64(1);                                                          \
        if ((P).stats && __builtin_amdgcn_mbcnt_hi((uint32_t)(ex_ >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ex_, 0u)) == 0) { \
            atomicAdd((P).stats + (slot), 1ull);                                                             \
            atomicAdd((P).stats + (slot) + 1, (unsigned long long)__popcll(ex_));                            \
        }                                                                                                    \
    } while (0)
#else
#define FLUX_SCENSUS(P, slot) ((void)0)
#endif
#endif
// -DFLUX_DEBUG_CENSUS=k (experiment builds, scripts/split_census.py): wave-level executions and active lanes of the code
// SECTIONS k, k+1, k+2 of the split kernel (section numbers at the call sites), in the statistics slots (10,11) (12,13) (14,15).
#ifndef FLUX_CENSUS_DEFINED
#define FLUX_CENSUS_DEFINED
#ifdef FLUX_DEBUG_CENSUS
#define FLUX_CENSUS(P, section)                                                                              \
    do {                                                                                                     \
        if ((section) >= FLUX_DEBUG_CENSUS && (section) < FLUX_DEBUG_CENSUS + 3) {                           \
            const unsigned long long ex_ = ballot64(1);                                                      \
            if ((P).stats && __builtin_amdgcn_mbcnt_hi((uint32_t)(ex_ >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ex_, 0u)) == 0) { \
                atomicAdd((P).stats + 10 + 2 * ((section) - FLUX_DEBUG_CENSUS), 1ull);                       \
                atomicAdd((P).stats + 11 + 2 * ((section) - FLUX_DEBUG_CENSUS), (unsigned long long)__popcll(ex_)); \
            }                                                                                                \
        }                                                                                                    \
    } while (0)
#else
#define FLUX_CENSUS(P, section) ((void)0)
#endif
#endif
// lap timer of the same experiment builds (-DFLUX_DEBUG_CLOCK): lap[slot] += cycles since the previous stamp, lap[7] = the
// previous stamp.  Product builds pass lap = nullptr and the stamps fold away.
__device__ __forceinline__ void lap_stamp(long long *lap, int slot) {
    if (lap) {
        const long long now = (long long)__builtin_readcyclecounter();
        lap[slot] += now - lap[7];
        lap[7] = now;
    }
}

struct V3 {
    double x, y, z;
};
__device__ __forceinline__ V3 mk(double x, double y, double z) { return V3{x, y, z}; }
__device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) {
    return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
__device__ __forceinline__ V3 normalize(V3 a) {
#if FLUX_FAST
    const double inv = fastmath::frsqrt(dot(a, a));
    return mk(a.x * inv, a.y * inv, a.z * inv);
#else
    double len = sqrt(dot(a, a));  // nalgebra normalize: component-wise divide by the norm
    return mk(a.x / len, a.y / len, a.z / len);
#endif
}

// trace.rs:72-80 + ray_direction trace.rs:44-51
__device__ __forceinline__ Ray primary_ray(const RenderParams &P, int row, int col, double2 sq,
                                           double2 lens) {
    double u = P.aps * (((double)col - P.half_w) + sq.x);
    double v = P.aps * (((double)(P.img_h - row) - P.half_h) + sq.y);
    double lpx = lens.x * P.lens_radius;
    double lpy = lens.y * P.lens_radius;
    double a = u * P.factor - lpx;
    double b = v * P.factor - lpy;
    // focal * W rounded on its own, as primary_ray_px gets it from pixel_consts: under `fp contract(fast)` the compiler may
    // otherwise fuse it into the subtraction (one rounding instead of two) here and not there, and the kernels that use the
    // two forms (refill / static: this one; split / bvh4: _px) would differ by an ulp in their primary rays -- their
    // "identical statistics, 1e-12" cross-checks must not hang on a compiler's choice (ADVICE round 4)
    double fwx = P.focal * P.Wx, fwy = P.focal * P.Wy, fwz = P.focal * P.Wz;
#if FLUX_FAST
    asm("" : "+v"(fwx), "+v"(fwy), "+v"(fwz));
#endif
    V3 dir = normalize(mk((a * P.Ux + b * P.Vx) - fwx, (a * P.Uy + b * P.Vy) - fwy, (a * P.Uz + b * P.Vz) - fwz));
    Ray r;
    r.dx = dir.x;
    r.dy = dir.y;
    r.dz = dir.z;
    r.ox = (P.ex + lpx * P.Ux) + lpy * P.Vx;
    r.oy = (P.ey + lpx * P.Uy) + lpy * P.Vy;
    r.oz = (P.ez + lpx * P.Uz) + lpy * P.Vz;
    return r;
}

// The same with the pixel's constants handed in: column and row offsets (col - half_w, (H - row) - half_h) and focal * W are
// the same for every sample of a pixel, i.e. wave-uniform where a wave owns a pixel; a kernel that is short of vector
// registers computes them once and keeps them in scalar registers (render_bvh4_kernel, render_split_kernel).  Same operations,
// same order, same roundings: focal * W is a value of its own in both forms (primary_ray pins it), so the two are bit-identical.
struct PixelConsts {
    double cu, cv, fwx, fwy, fwz;
};
__device__ __forceinline__ Ray primary_ray_px(const RenderParams &P, const PixelConsts &C, double2 sq, double2 lens) {
    double u = P.aps * (C.cu + sq.x);
    double v = P.aps * (C.cv + sq.y);
    double lpx = lens.x * P.lens_radius;
    double lpy = lens.y * P.lens_radius;
    double a = u * P.factor - lpx;
    double b = v * P.factor - lpy;
    V3 dir = normalize(mk((a * P.Ux + b * P.Vx) - C.fwx, (a * P.Uy + b * P.Vy) - C.fwy, (a * P.Uz + b * P.Vz) - C.fwz));
    Ray r;
    r.dx = dir.x;
    r.dy = dir.y;
    r.dz = dir.z;
    r.ox = (P.ex + lpx * P.Ux) + lpy * P.Vx;
    r.oy = (P.ey + lpx * P.Uy) + lpy * P.Vy;
    r.oz = (P.ez + lpx * P.Uz) + lpy * P.Vz;
    return r;
}

// a value every lane of the wave holds alike, moved to scalar registers
__device__ __forceinline__ double uniform_f64(double x) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(x)), __builtin_amdgcn_readfirstlane(__double2loint(x)));
}
__device__ __forceinline__ PixelConsts pixel_consts(const RenderParams &P, int row, int col) {
    return PixelConsts{uniform_f64((double)col - P.half_w), uniform_f64((double)(P.img_h - row) - P.half_h),
                       uniform_f64(P.focal * P.Wx), uniform_f64(P.focal * P.Wy), uniform_f64(P.focal * P.Wz)};
}

// path statistics (STATS builds only)
struct Stats {
    unsigned c[12];  // [10] / [11]: dielectric reflections / transmissions (include/flux_abi.h flux_ctx_stats)
};

// ---- extension: triangles (no reference counterpart; DESIGN.md "Triangles and the BVH") ----------
// Moeller-Trumbore, f64, two-sided; the CPU checker restates the same sequence of operations.
__device__ __forceinline__ bool tri_hit_v(V3 v0, V3 e1, V3 e2, const Ray &r, double &t) {
    const V3 d = mk(r.dx, r.dy, r.dz);
    const V3 p = cross(d, e2);
    const double det = dot(e1, p);
    if (det == 0.0) return false;
    const double inv = 1.0 / det;
    const V3 s = mk(r.ox - v0.x, r.oy - v0.y, r.oz - v0.z);
    const double u = dot(s, p) * inv;
    if (u < 0.0 || u > 1.0) return false;
    const V3 q = cross(s, e1);
    const double v = dot(d, q) * inv;
    if (v < 0.0 || u + v > 1.0) return false;
    t = dot(e2, q) * inv;
    return t > kTMin;
}
__device__ __forceinline__ bool tri_hit(const DevTri &T, const Ray &r, double &t) {
    return tri_hit_v(mk(T.v0x, T.v0y, T.v0z), mk(T.e1x, T.e1y, T.e1z), mk(T.e2x, T.e2y, T.e2z), r, t);
}

// extension: smooth meshes and vertex colours (DESIGN.md sections 5j and 5k; the spec: include/flux_abi.h flux_ctx_set_mesh_normals
// and flux_ctx_set_mesh_colors, tests/smooth_spec.py, tests/color_spec.py).
// The shading attributes of the hit of segment r on triangle `slot`.  Returned: the shading normal -- the stored facet normal, or,
// for a triangle whose mesh has corner normals, their interpolation at the hit's barycentrics, recomputed here from the DevTri record
// with tri_hit_v's own expressions (the traversal keeps no u, v: two registers less through its loop than carrying them would cost).
// (fr, fg, fb): the material's triple as the caller would read it, the three doubles at `records + index * stride` (a
// DevMaterial's fr, fg, fb, or the feature buffers' weight) -- times, for a triangle whose mesh has corner colours, their interpolation at the same barycentrics, clamped
// below at 0.  One barycentric computation serves both attributes, and both lie in the slot's one 128-B record.  Every reader of a
// triangle's normal or material colour calls this: the bounce and the facing test (shade_hit_fast, shade_hit), the feature buffers
// (first_hit_fields).
// The product sits inside the per-lane `colored` branch, with a read of the triple of its own, and every other lane reads the
// triple as it is behind it -- the stored normal's pattern.  So a context without a table (P.tri_attrs == nullptr: a scalar branch)
// runs the stored normal's and the triple's loads and nothing else: no product, no select.  (Multiplied in the caller under
// `P.tri_attrs != nullptr`, the compiler ran three products and six selects for every triangle hit and waited for the triple
// there: +1.6 % on configuration 5, which has no table.)  The coloured branch forms the triple's address from a copy of the index
// the compiler cannot see through: with one address for both reads it was computed in front of the scalar branch, and the wait
// for the triangle's material index with it -- ahead of the stored normal's loads instead of behind them.
__device__ __forceinline__ V3 tri_shading_normal(const RenderParams &P, const Ray &r, int slot, const char *records, uint32_t stride,
                                                 int index, double &fr, double &fg, double &fb) {
    const DevTri &T = P.tris[slot];
    bool flat = true, plain = true;
    V3 n;
    if (P.tri_attrs != nullptr) {
        const bool smooth = T.smooth != 0, colored = T.colored != 0;
        if (smooth || colored) {
            const V3 e1 = mk(T.e1x, T.e1y, T.e1z), e2 = mk(T.e2x, T.e2y, T.e2z);
            const V3 d = mk(r.dx, r.dy, r.dz);
            const V3 p = cross(d, e2);
            const V3 s = mk(r.ox - T.v0x, r.oy - T.v0y, r.oz - T.v0z);
#if FLUX_FAST
            const double inv = fastmath::fdiv(1.0, dot(e1, p));
#else
            const double inv = 1.0 / dot(e1, p);
#endif
            const double u = dot(s, p) * inv;
            const double v = dot(d, cross(s, e1)) * inv;
            // uniform base + 32-bit byte offset (the slot count keeps slot * 128 below 2^32, as for the DevTri records)
            const double *N = reinterpret_cast<const double *>(reinterpret_cast<const char *>(P.tri_attrs) +
                                                               (uint32_t)slot * (uint32_t)(kTriAttrDoubles * sizeof(double)));
            if (smooth) {
                const double w = (1.0 - u) - v;
                const V3 m = mk((w * N[0] + u * N[3]) + v * N[6], (w * N[1] + u * N[4]) + v * N[7], (w * N[2] + u * N[5]) + v * N[8]);
                const double l2 = (m.x * m.x + m.y * m.y) + m.z * m.z;
                flat = !(l2 >= 1e-24);  // (true for a NaN too: opposed corner normals and a degenerate hit keep the facet normal)
#if FLUX_FAST
                const double il = fastmath::frsqrt(l2);
                n = mk(m.x * il, m.y * il, m.z * il);
#else
                const double len = sqrt(l2);
                n = mk(m.x / len, m.y / len, m.z / len);
#endif
            }
            // (behind the normals: their eighteen registers are free again when the nine f32 colours arrive -- the same line)
            if (colored) {
                const float *K = reinterpret_cast<const float *>(N) + kTriColorFloat0;
                const double k0r = (double)K[0], k0g = (double)K[1], k0b = (double)K[2];
                // g1 = k1 - k0, g2 = k2 - k0, (k0 + u g1) + v g2, then maxNum against 0: a NaN and a rounding residue below 0 give 0
                const V3 c = mk(fmax((k0r + u * ((double)K[3] - k0r)) + v * ((double)K[6] - k0r), 0.0),
                                fmax((k0g + u * ((double)K[4] - k0g)) + v * ((double)K[7] - k0g), 0.0),
                                fmax((k0b + u * ((double)K[5] - k0b)) + v * ((double)K[8] - k0b), 0.0));
                int own = index;
                asm("" : "+v"(own));
                const double *triple = reinterpret_cast<const double *>(records + (uint32_t)own * stride);
                fr = triple[0] * c.x;
                fg = triple[1] * c.y;
                fb = triple[2] * c.z;
                plain = false;
            }
        }
    }
    // (the stored normal is read behind the interpolation, not in front of it: its six registers are not held across)
    if (flat) n = mk(T.nx, T.ny, T.nz);
    if (plain) {
        const double *triple = reinterpret_cast<const double *>(records + (uint32_t)index * stride);
        fr = triple[0];
        fg = triple[1];
        fb = triple[2];
    }
    return n;
}

// nearest-hit rule of Scene::hit (scene.rs:156-160 + Hit::compare common.rs:17-23) for candidates
// visited in ANY order: smaller t wins, equal t keeps the lower hit-order index (what min_by +
// Hit::compare give for an ordered scan)
__device__ __forceinline__ void consider(double t, int id, int slot, int &best, int &bslot, double &tb) {
    if (best < 0 || t < tb || (t == tb && id < best)) {
        best = id;
        bslot = slot;
        tb = t;
    }
}

// conservative slab test against an f32 box (already padded by the builder); inv* are finite
__device__ __forceinline__ bool box_hit(const float *lo, const float *hi, const Ray &r, double ix, double iy,
                                        double iz, double tb, bool have, double &tnear) {
    const double x0 = ((double)lo[0] - r.ox) * ix, x1 = ((double)hi[0] - r.ox) * ix;
    const double y0 = ((double)lo[1] - r.oy) * iy, y1 = ((double)hi[1] - r.oy) * iy;
    const double z0 = ((double)lo[2] - r.oz) * iz, z1 = ((double)hi[2] - r.oz) * iz;
    const double tn = fmax(fmax(fmin(x0, x1), fmin(y0, y1)), fmin(z0, z1));
    const double tf = fmin(fmin(fmax(x0, x1), fmax(y0, y1)), fmax(z0, z1));
    tnear = tn;
    return tn <= tf && tf >= 0.0 && (!have || tn <= tb);
}

template <bool STATS>
__device__ __forceinline__ void bvh_traverse(const RenderParams &P, const Ray &r, int *tstack, int stride,
                                             int &best, int &bslot, double &tb, Stats &st) {
    // reciprocal direction with zero components nudged to +-1e-300: no inf*0 = NaN in the slab test
    const double tiny = 1e-300;
    const double ix = 1.0 / (fabs(r.dx) < tiny ? copysign(tiny, r.dx) : r.dx);
    const double iy = 1.0 / (fabs(r.dy) < tiny ? copysign(tiny, r.dy) : r.dy);
    const double iz = 1.0 / (fabs(r.dz) < tiny ? copysign(tiny, r.dz) : r.dz);
    int sp = 0;
    int cur = 0;
    for (;;) {
        const DevNode N = P.nodes[cur];
        if (STATS) st.c[8]++;
        double tn0, tn1;
        bool h0 = box_hit(N.lo0, N.hi0, r, ix, iy, iz, tb, best >= 0, tn0);
        bool h1 = box_hit(N.lo1, N.hi1, r, ix, iy, iz, tb, best >= 0, tn1);
        if (h0 && N.child0 < 0) {  // leaf reference: ~((first << 3) | count)
            const int first = (~N.child0) >> 3, count0 = (~N.child0) & 7;
            for (int k = 0; k < count0; ++k) {
                double t;
                if (STATS) st.c[9]++;
                if (tri_hit(P.tris[first + k], r, t)) consider(t, P.tris[first + k].id, first + k, best, bslot, tb);
            }
            h0 = false;
        }
        if (h1 && N.child1 < 0) {
            const int first = (~N.child1) >> 3, count1 = (~N.child1) & 7;
            for (int k = 0; k < count1; ++k) {
                double t;
                if (STATS) st.c[9]++;
                if (tri_hit(P.tris[first + k], r, t)) consider(t, P.tris[first + k].id, first + k, best, bslot, tb);
            }
            h1 = false;
        }
        if (h0 && h1) {
            const bool near0 = tn0 <= tn1;
            tstack[sp * stride] = near0 ? N.child1 : N.child0;
            ++sp;
            cur = near0 ? N.child0 : N.child1;
        } else if (h0) {
            cur = N.child0;
        } else if (h1) {
            cur = N.child1;
        } else {
            if (sp == 0) break;
            --sp;
            cur = tstack[sp * stride];
        }
    }
}

// ---- disks (extension, include/flux_abi.h FLUX_SHAPE_DISK) ----
// Plane::hit's t (shapes.rs:135-152: the same operands in the same order), a hit iff t > T_MIN and the hit point q lies in the closed
// disk, |q - centre|^2 <= r^2.  q is formed as shade_hit forms the next segment's origin from (o, t, d) -- o + t d per component, one
// FMA each in FAST (contract(fast) fuses shade_hit's expression the same way), a product and a sum in STRICT -- so a path that is
// declared to hit the disk continues from a point that passed the test.  A non-finite t is never a hit: q is then infinite or NaN
// and fails the compare (rr is finite: abi.hip).
__device__ __forceinline__ bool disk_hit(const DevScanDisk &S, const Ray &r, double tmin, double &t) {
    const double num = (S.px - r.ox) * S.nx + (S.py - r.oy) * S.ny + (S.pz - r.oz) * S.nz;
    const double den = r.dx * S.nx + r.dy * S.ny + r.dz * S.nz;
    t = num / den;
#if FLUX_FAST
    const double qx = __builtin_fma(t, r.dx, r.ox), qy = __builtin_fma(t, r.dy, r.oy), qz = __builtin_fma(t, r.dz, r.oz);
#else
    const double qx = r.ox + t * r.dx, qy = r.oy + t * r.dy, qz = r.oz + t * r.dz;
#endif
    const double ex = qx - S.px, ey = qy - S.py, ez = qz - S.pz;
    return t > tmin && ex * ex + ey * ey + ez * ez <= S.rr;
}

// ---- boxes (extension, include/flux_abi.h FLUX_SHAPE_BOX; DESIGN.md §5d) ----
// The ray's side of BoundingBox::hit (shapes.rs:107,114,121): a_k = 1 / d_k, once per ray and not per box.  STRICT: IEEE division.
// FAST: flux_math.h's fdiv, which is defined for a finite normal divisor; a wave with a lane outside that (a zero -- whose +-inf the
// slabs' NaN rule needs --, a subnormal, a NaN) takes the IEEE quotient for that lane.
struct BoxRay {
    double ax, ay, az;
};
__device__ __forceinline__ double box_rcp(double d) {
#if FLUX_FAST
    double a = fastmath::fdiv(1.0, d);
    const bool plain = fabs(d) > 1e-290 && fabs(d) < 1e290;
    if (ballot64(!plain) != 0ull) a = plain ? a : 1.0 / d;
    return a;
#else
    return 1.0 / d;
#endif
}
__device__ __forceinline__ BoxRay box_ray(const Ray &r) { return BoxRay{box_rcp(r.dx), box_rcp(r.dy), box_rcp(r.dz)}; }
// BoundingBox::hit's slabs (shapes.rs:99-131) as a shape, in the order the spec writes them (include/flux_abi.h flux_shape).  max and
// min are the reference's own (shapes.rs:90-96: a > b ? a : b, a < b ? a : b): a ray parallel to a slab with its origin ON one of the
// slab's planes has 0 * inf = NaN there, which those forms drop for the x and y slabs (the slab bounds nothing) and hand through for
// the z slab (t0 or t1 is NaN, `t0 < t1` fails: a miss) -- box_z_nan_miss is the same arithmetic in front of a sphere.  The hit is the
// entry t0 if t0 > T_MIN, else the exit t1 if t1 > T_MIN.  `face` = 2 axis + (1: the face's outward normal is +e_axis), the first axis
// in x, y, z order whose own bound IS t: entry through the low face (normal -e) when a >= 0, exit through the high one.
__device__ __forceinline__ bool box_shape_hit(double c0x, double c0y, double c0z, double c1x, double c1y, double c1z, const Ray &r,
                                              const BoxRay &A, double tmin, double &t, int &face) {
    const bool px = A.ax >= 0.0, py = A.ay >= 0.0, pz = A.az >= 0.0;
    const double lox = (c0x - r.ox) * A.ax, hix = (c1x - r.ox) * A.ax;
    const double loy = (c0y - r.oy) * A.ay, hiy = (c1y - r.oy) * A.ay;
    const double loz = (c0z - r.oz) * A.az, hiz = (c1z - r.oz) * A.az;
    const double tx0 = px ? lox : hix, tx1 = px ? hix : lox;
    const double ty0 = py ? loy : hiy, ty1 = py ? hiy : loy;
    const double tz0 = pz ? loz : hiz, tz1 = pz ? hiz : loz;
    const double m0 = ty0 > tz0 ? ty0 : tz0, t0 = tx0 > m0 ? tx0 : m0;
    const double m1 = ty1 < tz1 ? ty1 : tz1, t1 = tx1 < m1 ? tx1 : m1;
    const bool entry = t0 > tmin;
    t = entry ? t0 : t1;
    const double bx = entry ? tx0 : tx1, by = entry ? ty0 : ty1;
    const int axis = bx == t ? 0 : (by == t ? 1 : 2);
    const bool pa = axis == 0 ? px : (axis == 1 ? py : pz);
    face = 2 * axis + (entry != pa ? 1 : 0);
    return t0 < t1 && t > tmin;
}

// ---- the conservative f32 sphere filter (flux_device.h DevScanSphere32), shared by FAST's scan and -- round 5 -- STRICT's ----
// Only a SUPERSET of the spheres a ray can hit comes out of it; the exact f64 test of the arithmetic in use decides every hit
// afterwards.  The ray's side of the test: u, o.u, 2 o and o.o (1 - 8e-6) in f32, each splatted into a pair.  (The records hold the
// NEGATED centres, so hb = o.u + (-p).u and c = o.o (1 - 8e-6) + (-p).(2 o) + ppr need no negation of the ray's side per pass; a
// product's rounding does not depend on which factor carries the sign, so the verdicts are those of the earlier p / -u / -2 o form.)
struct FilterRay32 {
    flux_f2 u_x, u_y, u_z, ou2, o2x2, o2y2, o2z2, oob2;
};
__device__ __forceinline__ FilterRay32 filter_ray32(double ox, double oy, double oz, double ux, double uy, double uz, double oo) {
    const float o2x = 2.0f * (float)ox, o2y = 2.0f * (float)oy, o2z = 2.0f * (float)oz;
    const float ufx = (float)ux, ufy = (float)uy, ufz = (float)uz;
    const float ouf = (float)(ox * ux + oy * uy + oz * uz);
    const float oob = (float)(oo * (1.0 - 8e-6));
    return FilterRay32{flux_f2{ufx, ufx}, flux_f2{ufy, ufy}, flux_f2{ufz, ufz}, flux_f2{ouf, ouf},
                       flux_f2{o2x, o2x}, flux_f2{o2y, o2y}, flux_f2{o2z, o2z}, flux_f2{oob, oob}};
}
// The same with o.u and o.o formed in f32 from the converted components (FAST's scan: six f64 operations and two conversions less per pass).
// Three more f32 roundings in each (<= 2e-7 of |o|^2 resp. |o||u|): inside the bias of 8e-6 of the squared magnitudes that already covers
// the 2.1e-6 of the filter's own roundings.  `oof` = o.o in f32, for the caller's range tests (inf / NaN for a component beyond f32).
__device__ __forceinline__ FilterRay32 filter_ray32_f(double ox, double oy, double oz, double ux, double uy, double uz, float &oof) {
    const float ofx = (float)ox, ofy = (float)oy, ofz = (float)oz;
    const float ufx = (float)ux, ufy = (float)uy, ufz = (float)uz;
    const float ouf = __builtin_fmaf(ofz, ufz, __builtin_fmaf(ofy, ufy, ofx * ufx));
    oof = __builtin_fmaf(ofz, ofz, __builtin_fmaf(ofy, ofy, ofx * ofx));
    const float oob = oof * (1.0f - 8e-6f);
    const float o2x = 2.0f * ofx, o2y = 2.0f * ofy, o2z = 2.0f * ofz;
    return FilterRay32{flux_f2{ufx, ufx}, flux_f2{ufy, ufy}, flux_f2{ufz, ufz}, flux_f2{ouf, ouf},
                       flux_f2{o2x, o2x}, flux_f2{o2y, o2y}, flux_f2{o2z, o2z}, flux_f2{oob, oob}};
}
// Candidate mask of spheres base .. base + lim - 1 (lim <= 32), sphere k at bit k; bits past `lim` are garbage (the caller masks).
// Candidate unless dq < 0 or (c > 0 and hb > 0), i.e. iff w = max(-dq, min(c, hb)) is negative (the biased values are never
// exactly 0): its SIGN BIT is the verdict.  Two spheres per packed-f32 instruction: 10 packed + 2 integer instructions per PAIR.
// Records are fetched in groups of 4 pairs (two s_load_dwordx16, one wait) and walked from the last sphere to the first, so
// that shifting each verdict in from the right leaves sphere k at bit k.  Slots past `lim` hold zeros.  (Hand-written
// v_pk_fma_f32 with op_sel modifiers instead of the splats the compiler makes of the ray's scalars -- 8 v_mov per pass -- was
// measured: +1.4 %, the asm blocks pin the schedule.)
// one pair of spheres: the two verdicts shifted into `cand` from the right
__device__ __forceinline__ void filter_pair_step(const FilterRay32 &F, const DevScanSphere32 &S, uint32_t &cand) {
    const flux_f2 hb = __builtin_elementwise_fma(S.px, F.u_x, __builtin_elementwise_fma(S.py, F.u_y, __builtin_elementwise_fma(S.pz, F.u_z, F.ou2)));
    const flux_f2 c = __builtin_elementwise_fma(S.px, F.o2x2, __builtin_elementwise_fma(S.py, F.o2y2, __builtin_elementwise_fma(S.pz, F.o2z2, F.oob2))) + S.ppr;
    const flux_f2 dq = __builtin_elementwise_fma(hb, hb, -c);
    // sign(max(-dq, min(c, hb))) = sign(-dq) & (sign(c) | sign(hb)): one three-input bit operation (v_bitop3_b32) per
    // sphere instead of a min and a max; the verdict is the sign bit, shifted into the mask: (cand << 1) | sign
    const uint32_t w1 = ~__float_as_uint(dq[1]) & (__float_as_uint(c[1]) | __float_as_uint(hb[1]));
    const uint32_t w0 = ~__float_as_uint(dq[0]) & (__float_as_uint(c[0]) | __float_as_uint(hb[0]));
    cand = __builtin_amdgcn_alignbit(cand, w1, 31);
    cand = __builtin_amdgcn_alignbit(cand, w0, 31);
}
__device__ __forceinline__ uint32_t sphere_filter32(const RenderParams &P, const FilterRay32 &F, int base, int lim) {
    uint32_t cand = 0;
    // pairs are walked from the last to the first.  A remainder of one or two pairs (demo2: 12 spheres = 6 pairs = a
    // group of four + two) is taken as a HALF group -- one s_load_dwordx16 -- instead of a whole group padded with
    // zeros (14 instructions per pair saved: 28 per pass on demo2); a remainder of three as a whole group.
    int pairs = (lim + 1) >> 1;
    const DevScanSphere32 *rec0 = P.fsph32 + (base >> 1);
    const int rem = pairs & 3;
    if (rem == 1 || rem == 2) {
        DevScanSphere32 S[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) S[j] = rec0[pairs - rem + j];
        filter_pair_step(F, S[1], cand);
        filter_pair_step(F, S[0], cand);
        pairs -= rem;
    } else if (rem == 3) {
        pairs += 1;  // its fourth pair is padding (zeros; masked off by the caller)
    }
    for (; pairs > 0; pairs -= 4) {
        DevScanSphere32 S[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) S[j] = rec0[pairs - 4 + j];
#pragma unroll
        for (int j = 3; j >= 0; --j) filter_pair_step(F, S[j], cand);
    }
    return cand;
}
// The same walk for a scene of at most 32 spheres (base = 0, lim = n_sph) with the half group's address, the end of the full groups and
// their number taken from the kernel arguments (abi.hip lays them out by the arithmetic above): three scalar loads where each pass formed
// them from n_sph with two dozen scalar instructions.
__device__ __forceinline__ uint32_t sphere_filter32_laid_out(const RenderParams &P, const FilterRay32 &F) {
    uint32_t cand = 0;
    const DevScanSphere32 *half = P.f32_half;
    if (half != nullptr) {
        DevScanSphere32 S[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) S[j] = half[j];
        filter_pair_step(F, S[1], cand);
        filter_pair_step(F, S[0], cand);
    }
    const DevScanSphere32 *g = P.f32_top;
    for (int n = P.f32_groups; n > 0; --n) {
        g -= 4;
        DevScanSphere32 S[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) S[j] = g[j];
#pragma unroll
        for (int j = 3; j >= 0; --j) filter_pair_step(F, S[j], cand);
    }
    return cand;
}

#if FLUX_FAST
// The ONE decision of BoundingBox::hit (shapes.rs:98-133) that the sphere quadratic does not imply.  The reference forms
// t0 = max(tx_min, max(ty_min, tz_min)) and t1 = min(tx_max, min(ty_max, tz_max)) with max(a,b) = a > b ? a : b and
// min(a,b) = a < b ? a : b (shapes.rs:90-96): a NaN in the x or y slab is dropped by those forms, a NaN in the Z slab
// comes out as t0 or t1, `t0 < t1` is false and Sphere::hit returns None before the quadratic runs (shapes.rs:173).  The z
// slab is NaN exactly when direction.z == +-0 (1/dz = +-inf) and the origin lies ON a z face of the box, (corner.z - oz)
// == 0: 0 * inf.  (Any other ray that hits the sphere passes the box: the sphere lies inside it.)  `k` = scan index.
__device__ __forceinline__ bool box_z_nan_miss(const RenderParams &P, const Ray &r, int k) {
    const DevShape &S = P.shapes[P.frec[k].orig_id];  // corners as Sphere::new forms them (shapes.rs:154-169, abi.hip)
    return r.oz == S.c0z || r.oz == S.c1z;
}

// Half-b of the sphere quadratic along the unit direction, with the contraction spelled out: the exact sphere test exists in
// three places (per-lane candidates, the wave-uniform `invert` spheres, the primary scan) and the tie rule between
// COINCIDENT spheres tested in different places (t == tb keeps the lower index) needs all of them to round alike; left to
// `fp contract(fast)` the compiler is free to fuse a*b + c*d + e*f differently from site to site (it did, once the code
// around one site changed: a coincident Reflective / Emissive pair of `invert` spheres then resolved to the wrong twin).
__device__ __forceinline__ double sphere_hb(double tx, double ty, double tz, double ux, double uy, double uz) {
    return __builtin_fma(tz, uz, __builtin_fma(ty, uy, tx * ux));
}

// Disks after the planes (FAST scans and the split kernel's primary scan): wave-uniform, operands in scalar registers, one scalar compare
// when the scene has none.  The general guarded update (`tb` means something only beside best >= 0: the first plane's peeled form leaves
// it as it comes under ENV_SHORT), and an equal t decided by the YAML index, not by scan order -- a disk listed before a coplanar plane
// still wins the tie.  `best` = hit record index (disk j: n_sph + n_pln + j), `best_id` its YAML index.
__device__ __forceinline__ void scan_disks(const RenderParams &P, const Ray &r, double tmin, int &best, int &best_id, double &tb) {
    for (int j = 0; j < P.n_dsk; ++j) {
        const DevScanDisk &S = P.fdsk[j];
        double t;
        if (disk_hit(S, r, tmin, t) && (best < 0 || t < tb || (t == tb && S.id < best_id))) {
            best = P.n_sph + P.n_pln + j;
            best_id = S.id;
            tb = t;
        }
    }
}

// Boxes after the disks, in the same places and by the same rules: wave-uniform, the corners in scalar registers, one scalar compare
// when the scene has none; the guarded update, an equal t decided by the YAML index.  The ray's reciprocals are formed once, in front of
// the loop.  `best` = the hit FACE's record, n_sph + n_pln + n_dsk + 6 j + face: behind the scan a box face is a plane.
__device__ __forceinline__ void scan_boxes(const RenderParams &P, const Ray &r, double tmin, int &best, int &best_id, double &tb) {
    if (P.n_box <= 0) return;
    const BoxRay A = box_ray(r);
    const int rec0 = P.n_sph + P.n_pln + P.n_dsk;
    for (int j = 0; j < P.n_box; ++j) {
        const DevScanBox &S = P.fbox[j];
        double t;
        int face;
        if (box_shape_hit(S.c0x, S.c0y, S.c0z, S.c1x, S.c1y, S.c1z, r, A, tmin, t, face) &&
            (best < 0 || t < tb || (t == tb && S.id < best_id))) {
            best = rec0 + 6 * j + face;
            best_id = S.id;
            tb = t;
        }
    }
}

// Which side of a sphere a ray met, without the normal.  Emissive::path_shade's facing test is -n.d > 0 with n = (pt - c) inv_rad and
// pt = o + t d: n.d = (hb + t) inv_rad along a unit d, and Sphere::hit's roots are t = -hb -+ e, e = sqrt(dq): n.d = -+e inv_rad.  So
// the test's answer is "the near root was taken" XOR "inv_rad < 0" -- unless e is rounding noise.  What the shading step computes for
// n.d differs from -+e inv_rad by the roundings of t (two operations and the square root's few ulp, of magnitudes below |o - c| + r),
// of the three components of pt - c and of the dot product: under the self-skip rule's guards (|o|^2 < 0.999e6, centres and radii
// below 1e3, hence t < 4e3) less than 20 x 1.1e-16 x 1e4 = 2.2e-11 |inv_rad|, plus t (|d|^2 - 1) < 4e3 x 4e-16.  The answer counts
// as known for dq >= 1e-12, e >= 1e-6: five orders of magnitude above that.  (Compared on the high word, as an integer: dq >= 0 here.)
constexpr int kFaceDqHi = 0x3d719799;                     // 1e-12 = 0x3d719799'812dea11: a high word above it
constexpr float kFaceEnvFront = 1.8446744073709552e19f;   // 0x5f800000: known, the far root (an `invert` sphere: front)
__device__ __forceinline__ float sphere_facing(double dq, bool near_root) {
    const float hq = __int_as_float(__double2hiint(dq));
    return near_root ? -hq : hq;
}
__device__ __forceinline__ bool facing_known(int facing) { return (facing & 0x7fffffff) > kFaceDqHi; }
// (inv_rad_hi: the high word of the record's inv_rad)
__device__ __forceinline__ bool facing_front(int facing, int inv_rad_hi) { return (facing ^ inv_rad_hi) < 0; }

// FAST: nearest analytic shape (spheres, planes, disks, boxes) of Scene::hit.  `best` = winning HIT RECORD index
// (scan order: spheres, then planes, then disks, then six face records per box) or -1; `tb` its distance.
// FACING (the split kernel's phase B with its hit queue): `*facing` tells the shading step which side of the winner the ray met, so that
// an Emissive hit's facing test needs no normal (sphere_facing above, shade_hit_fast).
template <bool ENV_SHORT = false, bool LDS_SCENE = false, bool MAX32 = false, bool TYP = false, int ZF = -1, bool FACING = false, int AXIS = 0>
__device__ __forceinline__ void scan_shapes_fast(const RenderParams &P, const Ray &r, int self, int &best, double &tb,
                                                 long long *lap = nullptr, const char *fsph_lds = nullptr, int *facing = nullptr) {
    (void)fsph_lds;  // LDS_SCENE (the split kernel): the block's LDS copy of the scan spheres for the per-lane gathers
    (void)facing;
    // FACING: the winner's discriminant dq / a as the high word of the double, with the sign bit set when Sphere::hit took the NEAR
    // root -- kept as a float so that the sign is a source modifier of the select --, or 0 = unknown: a plane, a disk, a box face, a
    // sphere decided by the exact code behind the candidate loop, and every winner of a pass outside the guards (ZF != 0; a scene
    // without P.self_skip).  ZF == 0 and P.self_skip are the self-skip rule's guards: |o|^2 < 0.999e6, centres and radii below 1e3.
    constexpr bool FACE = FACING && ZF == 0;
    float face = 0.0f;
    // FAST scan over the compact records of flux_device.h (DevScanPlane / DevScanSphere): `best` is the
    // winning shape's HIT RECORD index (scan order: spheres, planes, disks, a box's six faces), `best_id` its YAML index.
    // Planes first (Plane::hit, shapes.rs:135-152): IEEE division keeps the reference's +-inf / NaN
    // behaviour for rays parallel to the plane.  Planes come in YAML order, so an equal t never replaces.
    int best_id = -1;
    // T_MIN (constants.rs:4) from the kernel arguments: as a literal it was two scalar moves at each of the scan's five uses, every pass
    const double tmin = P.t_min;
    // The FIRST plane has nothing to compare with (`best` is -1 on entry, every caller): its verdict is one compare and one select, where
    // the loop's general step is three compares and two nested exec-masked regions with their moves.  The split kernel (ENV_SHORT) also
    // takes its distance as it comes: `tb` means something only beside best >= 0, and every later use there is guarded by that.
    // AXIS (the split kernel's TYP instantiations, one per axis, chosen by the launch from P.plane_axis; ZF = 0 only): the host has found
    // this plane's stored normal on that axis, so eight of the nine operations of the two dot products only carry exact zeros and
    // ones, and num = p_a - o_a, den = d_a give the same t bit for bit (flux_plane_axis.h) -- for a ray with d_a != 0, a finite
    // direction and a finite origin of ordinary size.  The caller's vote in front of ZF = 0 has established that for every lane of the
    // wave (split_rare_lanes); any other wave runs ZF = 1, this code with the general expressions.  A zero num needs no guard: t
    // is then a zero of either sign in both forms -- den is not zero -- and fails t > T_MIN whichever it is, and `tb` is read only
    // beside best >= 0.
    constexpr bool PLANE_AXIS = AXIS != kPlaneAxisNone && ZF == 0;
    int j0 = 0;
    if (P.n_pln > 0) {
        const DevScanPlane &S = P.fpln[0];
        double num, den;
        if (PLANE_AXIS) {
            plane_axis_num_den(AXIS, S.px, S.py, S.pz, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz, num, den);
        } else {
            num = (S.px - r.ox) * S.nx + (S.py - r.oy) * S.ny + (S.pz - r.oz) * S.nz;
            den = r.dx * S.nx + r.dy * S.ny + r.dz * S.nz;
        }
        // (AXIS: the vote has also put d_a where the division needs neither its operands scaled nor its result fixed up -- plane_div_admits,
        // plane_div_unscaled: the bits of num / den without three of its eleven instructions)
        const double t = PLANE_AXIS ? plane_div_unscaled(num, den) : num / den;
        const bool take = t > tmin;
        best = take ? P.n_sph : -1;
        best_id = S.id;
        tb = (ENV_SHORT || take) ? t : tb;
        j0 = 1;
    }
    for (int j = j0; j < P.n_pln; ++j) {
        const DevScanPlane &S = P.fpln[j];
        const double num = (S.px - r.ox) * S.nx + (S.py - r.oy) * S.ny + (S.pz - r.oz) * S.nz;
        const double den = r.dx * S.nx + r.dy * S.ny + r.dz * S.nz;
        const double t = num / den;
        if (t > tmin && (best < 0 || t < tb)) {
            best = P.n_sph + j;
            best_id = S.id;
            tb = t;
        }
    }
    // (TYP: the launch takes that instantiation only for a scene without disks -- the loop, even never entered, cost the split kernel
    // 1.2 % on demo2 in code it moved around)
    // (... and only for a scene without boxes)
    if (!TYP) {
        scan_disks(P, r, tmin, best, best_id, tb);
        scan_boxes(P, r, tmin, best, best_id, tb);
    }
    // Spheres, phase 1: wave-uniform index, operands in SGPRs, all lanes active -- only the half-b
    // discriminant of Sphere::hit (shapes.rs:176-184 with b = 2 hb along the unit direction: disc/4a = hb_u^2 - c)
    // plus the "sphere entirely behind the origin" rejection (c > 0 and hb > 0 => both roots negative).
    // BoundingBox::hit (shapes.rs:98-133,173) is a pre-filter whose answer the quadratic implies (the
    // sphere lies inside its box: a root t > T_MIN is inside the box's [t0,t1] and t1 >= t > T_MIN), so it
    // is not run.  Phase 2 takes sqrt only for each lane's OWN surviving candidates, lowest index first.
    // a = d.d (shapes.rs:177) is 1 to rounding for every direction this path produces from UNIT normals, but
    // plane normals are used as stored (never normalised, shapes.rs:135-152), and a reflection off a non-unit
    // normal is not a unit vector.  The quadratic is therefore solved along the unit direction u = d / |d|
    // (hb_u = hb/|d|, dq_u = hb_u^2 - c = dq/a, t = t_u / |d|): no per-sphere multiply by a.
    // Without such a plane (P.unit_dirs, set on the host; never for caller-supplied rays) every direction this path produces is
    // a unit vector to a few ulp -- normalised primaries, reflections about unit normals, lobe samples in orthonormal frames --
    // and is taken as the unit direction as it stands, as phase A of the split kernel does for primaries:
    // no rsqrt, no scaling (one wave-uniform branch).
    // TYP (the split kernel's instantiation for the usual scene, chosen by the launch: no non-unit plane normal, the self-skip rule in
    // force, ONE `invert` sphere and it is an Emissive environment, no disk): the scene's flags are compile-time constants here -- each was a
    // scalar load, a compare and a branch per pass, with the other side's code behind it
    const bool p_unit_dirs = TYP ? true : P.unit_dirs != 0;
    const bool p_env_short = TYP ? true : P.env_short != 0;
    const int p_n_uni = TYP ? 1 : P.n_uni;
    double rs = 1.0, ux = r.dx, uy = r.dy, uz = r.dz;
    if (!p_unit_dirs) {
        const double dd = r.dx * r.dx + r.dy * r.dy + r.dz * r.dz;
        rs = fastmath::frsqrt(dd);
        ux = r.dx * rs;
        uy = r.dy * rs;
        uz = r.dz * rs;
    }
    const bool zflat = r.dz == 0.0;  // box_z_nan_miss can apply to this lane
    // wave-uniform: the rule costs one compare per scan unless some lane has it.  (ZF = 0: the caller -- the split kernel -- has taken ONE
    // vote on the two rare cases of a pass, a lane with direction.z == 0 and a lane whose origin is beyond the filter's and the self-skip
    // rule's range (|o|^2 >= 0.999e6 in f32), and calls the instantiation that knows neither occurs: the zflat flag as two lane masks
    // and its three tests were ten scalar instructions a pass, the two range tests a compare and a select each per lane.)
    const bool any_zflat = ZF == 0 ? false : any64(zflat);
    // f32 operands of the conservative filter (flux_device.h DevScanSphere32): o, u, o.u and o.o (1 - 8e-6)
    // wave-uniform.  (TYP in the split kernel -- ENV_SHORT --: the launch has checked that the scene has its filter records, and the full
    // scan below is not compiled in: 198.7 -> 197.1 ms.  The mesh kernel measured 1.1 % SLOWER with the constant and keeps the test.)
    const bool f32_filter = (TYP && ENV_SHORT) ? true : P.fsph32 != nullptr;
    // (computed whether or not the filter is in use: under the wave-uniform `if` the compiler zero-initialised all eight for
    // the other arm in every pass)
    float oof;
    const FilterRay32 F32 = filter_ray32_f(r.ox, r.oy, r.oz, ux, uy, uz, oof);
    const bool big = ZF == 0 ? false : !(oof < 1e30f);  // beyond f32's safe range (or NaN): every sphere stays a candidate for this lane
    // The environment shortcut's f32 verdict (flux_env_verdict.h), ray side, from the filter's operands: three values for the code behind
    // the candidate loop.  ZF == 0 only: no lane's origin is beyond |o|^2 < 0.999e6 and none has direction.z == 0.
    constexpr bool ENV32 = ENV_SHORT && ZF == 0;
    EnvRay32 E32 = EnvRay32{0.0f, 0.0f, 0.0f};
    if (ENV32 && p_env_short && p_unit_dirs)
        E32 = env_ray32(P.env32, F32.o2x2[0], F32.o2y2[0], F32.o2z2[0], F32.u_x[0], F32.u_y[0], F32.u_z[0], F32.ou2[0], oof);
    // `self` = the sphere this ray leaves outwards (shade_hit), or -1.  Its own quadratic has c = |o - p|^2 - r^2 within
    // rounding of 0 and hb >= 0, so its roots are <= sqrt(|c|): with every magnitude below 1e3 (scene: P.self_skip;
    // previous segment: shade_hit; this origin: here) |c| < 1e-8 and the reference's test fails t > T_MIN = 5e-4 --
    // the sphere is dropped from this lane's candidates instead of being tested to that end
    if (ZF != 0 && !(oof < 0.999e6f)) self = -1;  // (|o|^2 in f32: relative error 2e-7, the threshold stays below 1e6)
    lap_stamp(lap, 2);
    // MAX32 (the split kernel's instantiation for scenes of at most 32 spheres, chosen by the launch): ONE group, so `base` is the
    // constant 0 and the loop's scalar induction variables (record pointers, counters: ~20 scalar instructions a pass) do not exist
    // (TYP: the scene has its environment sphere, so n_sph >= 1)
    const int n_groups_end = MAX32 ? ((TYP || P.n_sph > 0) ? 1 : 0) : P.n_sph;
    for (int base = 0; base < n_groups_end; base += 32) {
        const int lim = MAX32 ? P.n_sph : ((P.n_sph - base) < 32 ? (P.n_sph - base) : 32);
        uint32_t cand = 0;
        if (f32_filter) {
            cand = MAX32 ? sphere_filter32_laid_out(P, F32) : sphere_filter32(P, F32, base, lim);  // a superset; slots past `lim` are masked off below
            const uint32_t valid_bits = MAX32 ? P.f32_valid : (lim == 32 ? 0xffffffffu : (1u << lim) - 1u);
            cand = big ? valid_bits : (cand & valid_bits);
            const uint32_t sb = (uint32_t)(self - base);  // self = -1 or another block: no bit
            cand &= ~(sb < 32u ? 1u << sb : 0u);
        } else
        {
#pragma unroll 4
        for (int k = 0; k < lim; ++k) {  // unrolled: the scalar loads of 4 records are issued together
            const DevScanSphere S = P.fsph[base + k];
            const double tx = r.ox - S.px, ty = r.oy - S.py, tz = r.oz - S.pz;
            const double hb = sphere_hb(tx, ty, tz, ux, uy, uz);
            const double c = __builtin_fma(tx, tx, __builtin_fma(ty, ty, __builtin_fma(tz, tz, -S.rr)));
            const double dq = __builtin_fma(hb, hb, -c);
            // candidate unless dq < 0 or (c > 0 and hb > 0), decided on the sign/high words with 32-bit integer
            // compares (half the issue cost of f64 compares).  A superset is fine here (NaN, -0.0 and
            // subnormals may pass): phase 2 repeats the tests exactly.
            const int hq = __double2hiint(dq);
            const int hc = __double2hiint(c);
            const int hmin = min(hc, __double2hiint(hb));
            if (hq >= 0 && hmin <= 0) cand |= 1u << k;
        }
        }
        if (any_zflat) {  // rare: BoundingBox::hit's z-slab NaN turns these candidates into misses (box_z_nan_miss)
            if (zflat)
                for (uint32_t m = cand; m;) {
                    const int k = __builtin_ctz(m);
                    m &= m - 1;
                    if (box_z_nan_miss(P, r, base + k)) cand &= ~(1u << k);
                }
        }
        lap_stamp(lap, 3);
        // Phase 2: each lane's own candidates, lowest index first.  The record is a per-lane gather (32 contiguous bytes;
        // 32-bit byte offset from the uniform base -> saddr + voffset).  Requesting the NEXT candidate's record before the
        // current test was measured and dropped: +3 % VALU instructions, +1.6 % time (other waves cover the latency).
        uint32_t todo = cand;
        if (todo) {
            auto record = [&](int k) {
                if constexpr (LDS_SCENE)
                    return *reinterpret_cast<const DevScanSphere *>(fsph_lds + (uint32_t)(base + k) * (uint32_t)sizeof(DevScanSphere));
                else
                    return *reinterpret_cast<const DevScanSphere *>(
                        reinterpret_cast<const char *>(P.fsph) + (uint32_t)(base + k) * (uint32_t)sizeof(DevScanSphere));
            };
            int k = __builtin_ctz(todo);
            todo &= todo - 1;
            DevScanSphere Sk = record(k);
            for (;;) {
                FLUX_TRIP(P, 11);
                FLUX_CENSUS(P, 4);
                const double tx = r.ox - Sk.px, ty = r.oy - Sk.py, tz = r.oz - Sk.pz;
                const double hb = sphere_hb(tx, ty, tz, ux, uy, uz);
                const double c = __builtin_fma(tx, tx, __builtin_fma(ty, ty, __builtin_fma(tz, tz, -Sk.rr)));
                const double dq = __builtin_fma(hb, hb, -c);
                if (dq >= 0.0) {  // shapes.rs:181-183 (a NaN fails, as the reference's `t > T_MIN` on NaN)
                    const double e = fastmath::fsqrt_nonneg(dq);
                    double t = (-hb - e) * rs;             // shapes.rs:189
                    const float face_k = sphere_facing(dq, t > tmin);
                    if (!(t > tmin)) t = (-hb + e) * rs;  // shapes.rs:201
                    if (t > tmin) {
                        // min_by + Hit::compare: smaller t wins; equal t keeps the lower YAML index.  Spheres come in
                        // YAML order among themselves, so only a plane or a disk can hold an equal t with a higher index.
                        // (Flat -- no nested `if`s, the equal-t rule behind a vote -- was measured: three scalar instructions and two
                        // branches less per trip for one more compare, +0.4 % slower: profiles/r06_experiments/ab_m17_m18_m19_r06x.log.)
                        bool take = best < 0 || t < tb;
                        if (!take && t == tb && best >= P.n_sph) take = P.frec[base + k].orig_id < best_id;
                        if (take) {
                            best = base + k;
                            tb = t;
                            if (FACE) face = face_k;
                        }
                    }
                }
                if (!todo) break;
                k = __builtin_ctz(todo);
                todo &= todo - 1;
                Sk = record(k);
            }
        }
        lap_stamp(lap, 4);
    }
    // the `invert` spheres kept out of the filter (abi.hip): Sphere::hit with the record in SGPRs, every lane active.  They
    // come after the per-lane candidates, so the tie rule is spelled out: equal t keeps the lower YAML index.
    if (f32_filter) {
        for (int j = 0; j < p_n_uni; ++j) {
            FLUX_CENSUS(P, 5);
            const int k = P.uni_idx[j];
            if (ENV32 && p_env_short && p_unit_dirs) {
                // The shortcut below, decided in f32 first: per lane "the environment wins", "loses" or "undecided", each from the sign
                // of |o + tb u - p|^2 - r^2 with a margin that covers the f32 roundings and the f64 shortcut's own "too close to call"
                // band (flux_env_verdict.h).  A wave without an undecided lane takes the verdicts -- they are the f64 shortcut's for
                // every lane, and it would have passed its vote -- for one conversion and four f32 operations in place of 16 f64
                // operations and 5 f64 compares; any other wave runs the code below as it stands.  (The votes as lane masks of the
                // compares, as below.  A NaN fails every compare: undecided.)
                float g_lo, g_hi;
                env_g32(E32, (float)tb, g_lo, g_hi);
                if ((ballot64(!(E32.cp < P.env32.deep)) | (ballot64(best >= 0) & ballot64(!(g_lo > 0.0f)) & ballot64(!(g_hi < 0.0f)))) == 0ull) {
                    if (best < 0 || g_lo > 0.0f) {
                        best = k;
                        tb = 2.0 * P.env_radius;
                        if (FACE) face = kFaceEnvFront;
                    }
                    continue;
                }
            }
            // (TYP: the one such sphere's record is in the kernel arguments)
            const DevScanSphere S = TYP ? DevScanSphere{P.env_px, P.env_py, P.env_pz, P.env_rr} : P.fsph[k];
            const double tx = r.ox - S.px, ty = r.oy - S.py, tz = r.oz - S.pz;
            const double hb = sphere_hb(tx, ty, tz, ux, uy, uz);
            const double c = __builtin_fma(tx, tx, __builtin_fma(ty, ty, __builtin_fma(tz, tz, -S.rr)));
            const double dq = __builtin_fma(hb, hb, -c);
            if (ENV_SHORT && p_env_short && p_unit_dirs && !any_zflat) {
                // The scene's one `invert` sphere, and it is Emissive (abi.hip); directions are unit vectors (rs = 1).  Its far
                // root is t_env = -hb + e, e = sqrt(dq).  For an origin inside by a margin (c < -4 r T_MIN: the surface is at
                // least |c| / 2r away in every direction, so t_env > 2 T_MIN) it is a hit, its near root is negative, and
                // Emissive::path_shade's facing test (-n.d = e / r) holds whatever t is.  All that is left to decide is whether
                // it is nearer than the best hit so far, t_env < tb  <=>  e < s = tb + hb  <=>  s > 0 and dq < s^2: no square
                // root.  Within 1e-9 of equality (where the reference's own rounding of t_env, or its tie rule, would decide)
                // -- or for an origin not clearly inside -- the wave takes the exact code below instead, so the decisions are
                // the exact code's.  The winner's distance is not computed: tb becomes an upper bound of it, which the facing
                // test accepts (shade_hit: -n.d = (hb + t) / r > 0 for every t >= t_env).  Split kernel only: a mesh kernel
                // needs the true distance to bound its traversal.
                const bool deep = c < P.env_deep;
                const double s = tb + hb;
                const double s2 = s * s;
                const bool close = fabs(dq - s2) <= P.env_eps * (dq + s2);  // (1e-9, from the kernel arguments)
                // (the vote as lane masks of the three compares, combined in scalar registers: a ballot of a compare IS the compare's
                // result, a ballot of a boolean expression goes through a 0/1 select and a second compare -- two VALU instructions a trip)
                if (((ballot64(!deep)) | (ballot64(best >= 0) & ballot64(close))) == 0ull) {
                    if (best < 0 || (s > 0.0 && dq < s2)) {
                        best = k;
                        tb = 2.0 * P.env_radius;  // >= -hb + e for an origin inside: |hb| <= |o - p| < r and e <= r (a wave-uniform value: no per-lane arithmetic)
                        if (FACE) face = kFaceEnvFront;  // the far root of an `invert` sphere: the facing test holds (above)
                    }
                    continue;
                }
            }
            const double e = fastmath::fsqrt_nonneg(__builtin_fmax(dq, 0.0));
            double t = (-hb - e) * rs;             // shapes.rs:189
            if (!(t > tmin)) t = (-hb + e) * rs;  // shapes.rs:201
            bool ok = dq >= 0.0 && t > tmin;      // shapes.rs:181-183 (NaN fails both, as in the reference)
            if (any_zflat) {
                if (zflat && box_z_nan_miss(P, r, k)) ok = false;
            }
            if (ok) {
                bool take = best < 0 || t < tb;
                if (!take && t == tb) take = best >= P.n_sph ? P.frec[k].orig_id < best_id : k < best;
                if (take) {
                    best = k;
                    tb = t;
                    if (FACE) face = 0.0f;
                }
            }
        }
    }
    if (FACING) *facing = (FACE && (TYP || P.self_skip != 0)) ? __float_as_int(face) : 0;
}
#endif

// Scene::hit (scene.rs:156-160): nearest of all shapes, ties keep the lower index.  Returns -1 on miss.
template <bool STATS, bool TRIS>
__device__ __forceinline__ int scene_hit(const RenderParams &P, const Ray &r, int self, double &t_out, int &slot_out,
                                         int *tstack, int stride, Stats &st) {
    int best = -1;
    int bslot = -1;
    double tb = 0.0;
#if FLUX_FAST
    scan_shapes_fast(P, r, self, best, tb);
    const int best_rec = best;
    if (TRIS) best = best >= 0 ? 0 : -1;  // triangle ids follow every shape id: a shape wins any tie
#else
    // BoundingBox::hit's reciprocals depend on the ray only (shapes.rs:107,114,121)
    const double ax = 1.0 / r.dx, ay = 1.0 / r.dy, az = 1.0 / r.dz;
    const double a = r.dx * r.dx + r.dy * r.dy + r.dz * r.dz;  // shapes.rs:177
    const double denom = 2.0 * a;                               // shapes.rs:187
    // Round 5: the candidates of the sphere tests come from the conservative f32 filter (sphere_filter32 above, FAST's).  A hit
    // needs BoundingBox::hit AND the quadratic to say yes (shapes.rs:173-214); the filter passes every sphere whose quadratic can
    // say yes -- a superset with a margin of 8e-6 of the squared magnitudes, eleven orders above f64 rounding in any operation
    // order --, so a sphere it rejects is a miss whatever its box test says, and neither test needs to be run for it.  For the
    // spheres it passes, both run exactly as the reference has them, box first: every value that reaches the image is computed
    // by the reference's operations in the reference's order, and the frames are the same bits as with the full scan
    // (tests/test_gpu_parity.py::test_strict_filter_equals_the_full_scan).
    // What it saves: the box test of the ~11 of demo2's 12 spheres a ray comes nowhere near -- 34 VALU instructions each, per
    // ray segment: two fifths of the STRICT kernel's instructions.
    // `invert` spheres (up to two: abi.hip) never pass the filter; they are tested for all lanes with scalar operands, as every
    // sphere was.  Planes as before.  Scenes the filter is not defined for (a coordinate beyond 1e15) keep the full scan.
    const auto box_hit_strict = [&](const DevShape &S) {  // BoundingBox::hit: shapes.rs:98-133
        double lox = (S.c0x - r.ox) * ax, hix = (S.c1x - r.ox) * ax;
        double loy = (S.c0y - r.oy) * ay, hiy = (S.c1y - r.oy) * ay;
        double loz = (S.c0z - r.oz) * az, hiz = (S.c1z - r.oz) * az;
        double tx_min = ax >= 0.0 ? lox : hix, tx_max = ax >= 0.0 ? hix : lox;
        double ty_min = ay >= 0.0 ? loy : hiy, ty_max = ay >= 0.0 ? hiy : loy;
        double tz_min = az >= 0.0 ? loz : hiz, tz_max = az >= 0.0 ? hiz : loz;
        const double t0 = __builtin_fmax(tx_min, __builtin_fmax(ty_min, tz_min));  // (see the full scan below for the NaN argument)
        const double t1 = __builtin_fmin(tx_max, __builtin_fmin(ty_max, tz_max));
        return t0 < t1 && t1 > kTMin && !__builtin_isunordered(tz_min, tz_max);
    };
    const auto sphere_hit_strict = [&](const DevShape &S) {  // Sphere::hit: shapes.rs:176-214
        V3 temp = mk(r.ox - S.px, r.oy - S.py, r.oz - S.pz);
        double b = 2.0 * (temp.x * r.dx + temp.y * r.dy + temp.z * r.dz);
        double c = dot(temp, temp) - S.rr;
        double disc = b * b - 4.0 * a * c;
        if (!(disc < 0.0)) {
            double e = sqrt(disc);
            double t = (-b - e) / denom;
            bool ok = t > kTMin;
            if (!ok) {
                t = (-b + e) / denom;
                ok = t > kTMin;
            }
            if (ok) consider(t, S.pad0, -1, best, bslot, tb);
        }
    };
    if (P.fsph32 != nullptr) {
        for (int j = 0; j < P.n_pln; ++j) {  // Plane::hit: shapes.rs:135-152
            const DevScanPlane &S = P.fpln[j];
            double num = (S.px - r.ox) * S.nx + (S.py - r.oy) * S.ny + (S.pz - r.oz) * S.nz;
            double den = r.dx * S.nx + r.dy * S.ny + r.dz * S.nz;
            double t = num / den;
            if (t > kTMin) consider(t, S.id, -1, best, bslot, tb);
        }
        for (int j = 0; j < P.n_dsk; ++j) {  // disks (extension): consider() applies the tie rule by YAML index
            const DevScanDisk &S = P.fdsk[j];
            double t;
            if (disk_hit(S, r, kTMin, t)) consider(t, S.id, -1, best, bslot, tb);
        }
        for (int j = 0; j < P.n_box; ++j) {  // boxes (extension): the hit face travels in the slot, -2 - face (shade_hit)
            const DevScanBox &S = P.fbox[j];
            double t;
            int face;
            if (box_shape_hit(S.c0x, S.c0y, S.c0z, S.c1x, S.c1y, S.c1z, r, BoxRay{ax, ay, az}, kTMin, t, face))
                consider(t, S.id, -2 - face, best, bslot, tb);
        }
        // the filter's ray: unit direction (2-ulp reciprocal square root: it only feeds the conservative test), o.o
        const double rs = fastmath::frsqrt(a);
        const double ux = r.dx * rs, uy = r.dy * rs, uz = r.dz * rs;
        const double oo = r.ox * r.ox + r.oy * r.oy + r.oz * r.oz;
        // beyond f32's safe range, or a NaN anywhere in the ray: every sphere stays a candidate (negated comparisons)
        const bool big = !(oo < 1e30) || !(a > 1e-280 && a < 1e280);
        const FilterRay32 F32 = filter_ray32(r.ox, r.oy, r.oz, ux, uy, uz, oo);
        for (int base = 0; base < P.n_sph; base += 32) {
            const int lim = (P.n_sph - base) < 32 ? (P.n_sph - base) : 32;
            const uint32_t valid_bits = lim == 32 ? 0xffffffffu : (1u << lim) - 1u;
            uint32_t cand = sphere_filter32(P, F32, base, lim);
            cand = big ? valid_bits : (cand & valid_bits);
            for (int j = 0; j < P.n_uni; ++j) {  // (their filter records never pass; a lane that is `big` must not test them twice)
                const uint32_t ub = (uint32_t)(P.uni_idx[j] - base);
                cand &= ~(ub < 32u ? 1u << ub : 0u);
            }
            FLUX_SCENSUS(P, 10);
            while (cand) {
                FLUX_SCENSUS(P, 12);
                const int k = __builtin_ctz(cand);
                cand &= cand - 1;
                const DevShape &S = *reinterpret_cast<const DevShape *>(reinterpret_cast<const char *>(P.sshapes) +
                                                                         (uint32_t)(base + k) * (uint32_t)sizeof(DevShape));
                if (box_hit_strict(S)) {
                    FLUX_SCENSUS(P, 14);
                    sphere_hit_strict(S);
                }
            }
        }
        for (int j = 0; j < P.n_uni; ++j) {
            const DevShape &S = P.sshapes[P.uni_idx[j]];  // wave-uniform: scalar operands
            if (box_hit_strict(S)) sphere_hit_strict(S);
        }
    } else
    // The reference scans every shape and runs BoundingBox::hit before each sphere (shapes.rs:173).
    // Same tests, regrouped for the machine: phase 1 walks the shapes with a wave-uniform index
    // (operands in SGPRs, all lanes active) doing the plane test and only the box test of each sphere;
    // phase 2 runs the sphere quadratic for each lane's OWN candidates, lowest index first, so the
    // sqrt/divides execute with most lanes active instead of once per shape under a sparse mask.
    // consider() applies min_by's rule order-independently (smaller t; equal t -> lower index).
    for (int base = 0; base < P.n_shapes; base += 32) {
        const int lim = (P.n_shapes - base) < 32 ? (P.n_shapes - base) : 32;
        uint32_t cand = 0;
#if FLUX_STRICT_SCAN_UNROLL > 1
#pragma unroll FLUX_STRICT_SCAN_UNROLL
#endif
        for (int k = 0; k < lim; ++k) {
            const DevShape &S = P.shapes[base + k];
            if (S.kind == kShapeSphere) {
                // BoundingBox::hit: shapes.rs:98-133
                double lox = (S.c0x - r.ox) * ax, hix = (S.c1x - r.ox) * ax;
                double loy = (S.c0y - r.oy) * ay, hiy = (S.c1y - r.oy) * ay;
                double loz = (S.c0z - r.oz) * az, hiz = (S.c1z - r.oz) * az;
                double tx_min = ax >= 0.0 ? lox : hix, tx_max = ax >= 0.0 ? hix : lox;
                double ty_min = ay >= 0.0 ? loy : hiy, ty_max = ay >= 0.0 ? hiy : loy;
                double tz_min = az >= 0.0 ? loz : hiz, tz_max = az >= 0.0 ? hiz : loz;
                // The reference's max(a,b) = a > b ? a : b and min(a,b) = a < b ? a : b (shapes.rs:90-96) against the machine's
                // v_max_f64 / v_min_f64 (IEEE maxNum / minNum), for what the VERDICT t0 < t1 && t1 > T_MIN can see:
                //   * no NaN among the operands: the same value up to the sign of a zero, which no comparison sees;
                //   * a NaN in the x or y slab: the reference's forms drop it (a NaN `a` loses every a > b; in m0 the y slab is
                //     `a`, in t0 the x slab is) -- maxNum / minNum drop it too;
                //   * a NaN in the Z slab: the reference's forms hand it through (it is `b` of the inner call, and the inner
                //     result is `b` of the outer), t0 or t1 is NaN and the verdict is false -- maxNum would drop it.  One
                //     unordered compare of (tz_min, tz_max) restores that.
                // Two instructions per max / min less (compare + two selects each), the same verdict bit for bit.
                const double t0 = __builtin_fmax(tx_min, __builtin_fmax(ty_min, tz_min));
                const double t1 = __builtin_fmin(tx_max, __builtin_fmin(ty_max, tz_max));
                if (t0 < t1 && t1 > kTMin && !__builtin_isunordered(tz_min, tz_max)) cand |= 1u << k;
            } else if (S.kind == kShapePlane) {
                // Plane::hit: shapes.rs:135-152 (normal stored in c0)
                double num = (S.px - r.ox) * S.c0x + (S.py - r.oy) * S.c0y + (S.pz - r.oz) * S.c0z;
                double den = r.dx * S.c0x + r.dy * S.c0y + r.dz * S.c0z;
                double t = num / den;
                if (t > kTMin) consider(t, base + k, -1, best, bslot, tb);
            } else if (S.kind == kShapeDisk) {
                // disk (extension): centre in p, normal in c0, r^2 in rr
                const DevScanDisk D = {S.px, S.py, S.pz, S.c0x, S.c0y, S.c0z, base + k, 0, S.rr};
                double t;
                if (disk_hit(D, r, kTMin, t)) consider(t, base + k, -1, best, bslot, tb);
            } else {
                // box (extension): corners in c0 / c1; the hit face travels in the slot, -2 - face (shade_hit)
                double t;
                int face;
                if (box_shape_hit(S.c0x, S.c0y, S.c0z, S.c1x, S.c1y, S.c1z, r, BoxRay{ax, ay, az}, kTMin, t, face))
                    consider(t, base + k, -2 - face, best, bslot, tb);
            }
        }
        while (cand) {
            const int k = __builtin_ctz(cand);
            cand &= cand - 1;
            const DevShape *S = P.shapes + (base + k);  // per-lane gather of 32 contiguous bytes
            // Sphere::hit: shapes.rs:176-214
            V3 temp = mk(r.ox - S->px, r.oy - S->py, r.oz - S->pz);
            double b = 2.0 * (temp.x * r.dx + temp.y * r.dy + temp.z * r.dz);
            double c = dot(temp, temp) - S->rr;
            double disc = b * b - 4.0 * a * c;
            if (!(disc < 0.0)) {
                double e = sqrt(disc);
                double t = (-b - e) / denom;
                bool ok = t > kTMin;
                if (!ok) {
                    t = (-b + e) / denom;
                    ok = t > kTMin;
                }
                if (ok) consider(t, base + k, -1, best, bslot, tb);
            }
        }
    }
#endif
    if (TRIS) {
        // triangles continue the scan with hit-order indices n_shapes + k
        if (P.bvh_stack > 0) {
            bvh_traverse<STATS>(P, r, tstack, stride, best, bslot, tb, st);
        } else {
            for (int k = 0; k < P.n_tris; ++k) {  // brute force, wave-uniform index
                double t;
                if (STATS) st.c[9]++;
                if (tri_hit(P.tris[k], r, t)) consider(t, P.tris[k].id, k, best, bslot, tb);
            }
        }
    }
    t_out = tb;
    slot_out = bslot;
#if FLUX_FAST
    return (TRIS && bslot >= 0) ? best : best_rec;  // shape: hit-record index; triangle: its id (slot_out set)
#else
    return best;
#endif
}

// to_unit_hemi: samplers/src/lib.rs:133-142
__device__ __forceinline__ V3 to_unit_hemi(double2 p, double inv_e1) {
#if FLUX_FAST
    double sin_phi, cos_phi;
    fastmath::fsincos2pi(p.x, sin_phi, cos_phi);  // phi = 2 pi x, reduced exactly by quarter turns
    FLUX_STAGE();
    const double cos_theta = fastmath::fpow_pos(1.0 - p.y, inv_e1);
    FLUX_STAGE();
    const double sin_theta = fastmath::fsqrt(1.0 - cos_theta * cos_theta);
    // the reference normalises this vector; its length is 1 to rounding (sin^2 + cos^2), so the
    // divide by ~1.0 changes nothing above an ulp and is not repeated here
    return mk(sin_theta * cos_phi, sin_theta * sin_phi, cos_theta);
#else
    double phi = 2.0 * kPi * p.x;
    double sin_phi, cos_phi;
    sincos(phi, &sin_phi, &cos_phi);
    double cos_theta = pow(1.0 - p.y, inv_e1);
    double sin_theta = sqrt(1.0 - cos_theta * cos_theta);
    return normalize(mk(sin_theta * cos_phi, sin_theta * sin_phi, cos_theta));
#endif
}

// ---- dielectric (extension, include/flux_abi.h FLUX_MAT_DIELECTRIC; DESIGN.md §5c) ----
// One bounce of the spec in the order it is written: n the shading normal the other materials use, d the segment's direction, ri the
// refraction index, u the z of hemi_sets[set][depth-1][sample].  Returns true for a reflection (weight 1; total internal reflection
// included), false for a transmission (weight transmit_color); wi the new direction, a unit vector to rounding.  STRICT: IEEE
// division and square root, no contraction; FAST: the same operations under contract(fast).
__device__ __forceinline__ bool dielectric_dir(V3 n, V3 d, double ri, double u, V3 &wi) {
    const double ln = sqrt(n.x * n.x + n.y * n.y + n.z * n.z), ld = sqrt(d.x * d.x + d.y * d.y + d.z * d.z);
    const V3 nh = mk(n.x / ln, n.y / ln, n.z / ln), dh = mk(d.x / ld, d.y / ld, d.z / ld);
    double c = -(dh.x * nh.x + dh.y * nh.y + dh.z * nh.z);
    double eta = ri;
    V3 m = nh;
    if (!(c > 0.0)) {  // arriving from the inside (the side the normal points away from)
        eta = 1.0 / ri;
        m = mk(-nh.x, -nh.y, -nh.z);
        c = -c;
    }
    const double k = 1.0 - (1.0 - c * c) / (eta * eta);
    double F = 1.0, ct = 0.0;  // k < 0: total internal reflection
    if (!(k < 0.0)) {
        ct = sqrt(k);
        const double rs = (c - eta * ct) / (c + eta * ct);
        const double rp = (eta * c - ct) / (eta * c + ct);
        F = (rs * rs + rp * rp) / 2.0;
    }
    if (u <= F) {
        const double c2 = 2.0 * c;
        wi = mk(dh.x + c2 * m.x, dh.y + c2 * m.y, dh.z + c2 * m.z);
        return true;
    }
    const double a = c / eta - ct;
    wi = mk(dh.x / eta + a * m.x, dh.y / eta + a * m.y, dh.z / eta + a * m.z);
    return false;
}

// Per-lane path state.
struct Path {
    Ray r;
    int depth;    // 1-based depth of the segment being traced (scene.rs:162)
    int nb;       // entries on this lane's (f,s) stack (strict) / bounces so far (fast)
    double2 sq;   // pixel_sets[set][i] (also the glossy lobe sample, brdf.rs:64)
#if FLUX_FAST
    double tr, tg, tb;  // throughput: product of (f * s) over the bounces so far
    int self;           // hit-record index of the sphere this segment leaves outwards (scan_shapes_fast), else -1
    int mat;            // material index (RenderParams::mats) of the bounce shade_hit just recorded (render_bvh4_kernel's list)
#endif
};
__device__ __forceinline__ int path_self(const Path &p) {
#if FLUX_FAST
    return p.self;
#else
    return -1;
#endif
}

__device__ __forceinline__ void path_begin(Path &p) {
    p.depth = 1;
    p.nb = 0;
#if FLUX_FAST
    p.tr = p.tg = p.tb = 1.0;
    p.self = -1;
    p.mat = 0;
#endif
}

#if FLUX_FAST
// A hit record's entry of the lobe-frame table (RenderParams::lobe_frame) as the uniform step holds it: in scalar registers, read
// beside the record itself (analytic_hit_fields<UNI>).  on: the context has the table and the record's shape stores its normal, which
// (nx, ny, nz) then is -- the record's own words, never a copy in vector registers.
// LF, the table's part in an instantiation's uniform step: kLobeOff -- none, the parent's code; kLobeEarly -- the entry's loads go out
// with the record's own, so that one wait covers both (TYP); kLobeLate -- they go out in the arm itself: a wait of its own, but twelve
// scalar registers held for a shorter time, which the instantiations outside TYP do not have to spare (split_lobe_frames).
constexpr int kLobeOff = 0, kLobeEarly = 1, kLobeLate = 2;
struct LobeFrameU {
    double b1x = 0.0, b1y = 0.0, b1z = 0.0, b2x = 0.0, b2y = 0.0, b2z = 0.0;
    double nx = 0.0, ny = 0.0, nz = 0.0;
    bool on = false;
};
typedef const __attribute__((address_space(4))) double *LobeFrameScalar;

// The end of a bounce: the weight into the throughput (FIRST: the throughput is still exactly 1, so it BECOMES the weight) and the
// child ray from `pt` along `wi`.
template <bool FIRST>
__device__ __forceinline__ void advance_path(Path &p, V3 pt, V3 wi, double fr, double fg, double fb, double scale) {
    if (FIRST) {
        p.tr = fr * scale;
        p.tg = fg * scale;
        p.tb = fb * scale;
    } else {
        p.tr *= fr * scale;
        p.tg *= fg * scale;
        p.tb *= fb * scale;
    }
    p.nb++;
    p.depth++;
    p.r.ox = pt.x;
    p.r.oy = pt.y;
    p.r.oz = pt.z;
    p.r.dx = wi.x;
    p.r.dy = wi.y;
    p.r.dz = wi.z;
}

// The bounce of the FAST arithmetic -- the lobe code and the ONLY update of the loop-carried path state --, shared by the two forms of
// the shading step (shade_hit_fast below: after the join of the miss / emitter exits; shade_hit: after its early returns).  One copy:
// a fix made here reaches every kernel (ADVICE round 4).
// fr / fg / fb: the bounce weight of an analytic shape's hit record (DevHitRec: f (n.wi)/pdf in closed form), or the plain f of a
// triangle's DevMaterial (is_tri: the Matte factor 1 / INV_PI is then applied here).  ax / az: the lobe frame's helper vector (DevHitRec).
// FIRST: the path's first bounce (phase A of the split kernel): its throughput is still exactly 1, so it BECOMES the weight (1.0 * w = w
// bit for bit) instead of being multiplied by it.
// UNI: `hit` and everything read from its record (kind, n of a stored-normal shape, fr / fg / fb, ax / az, unit_n, convex) are
// wave-uniform (shade_primary_hits): the tests on them are scalar branches, and what a branch makes an identity -- the (c1, c2) selects,
// a Matte bounce's x 1.0, the normalisation's select, dot(n, wi) of a shape that is not a convex sphere -- is not executed.  Every
// operation that IS executed has the operands and the order of the general form.
// UNI with lf.on, a Matte hit: w = n is the record's stored normal, so the frame (b1, b2) is a constant of the record and comes from
// the table (lf) instead of two cross products and a normalisation of wave-uniform values.  The arm forms wi itself -- the general
// form's one product and two fused multiply-adds per component, with the frame and the normal as scalar operands -- and leaves: it
// shares no value with the computing arm, so nothing of the frame is ever copied into vector registers.
template <bool STATS, bool TRIS, bool TYP = false, bool FIRST = false, bool UNI = false, int LF = kLobeOff>
__device__ __forceinline__ void fast_bounce(const RenderParams &P, Path &p, uint32_t set, uint32_t i, int hit, int slot, double t, V3 n,
                                            V3 d, V3 pt, int kind, double fr, double fg, double fb, double m_inv_e1, double ax, double az,
                                            bool unit_n, bool convex, bool is_tri, Stats &st, int cz, const LobeFrameU &lf = LobeFrameU()) {
    (void)cz;
    (void)lf;
    // (TYP: the scene's flags as constants, see scan_shapes_fast)
    const bool p_glossy_long = TYP ? false : P.glossy_long != 0;
    const bool p_unit_dirs = TYP ? true : P.unit_dirs != 0;
    const bool p_self_skip = TYP ? true : P.self_skip != 0;
    // FAST: the two sampled lobes share one frame construction and one transform.
    //   Lambertian (brdf.rs:22-27): w = n,  v = normalize((0.0034, 1, 0.0071) x w),  u = v x w,
    //                               wi = normalize(hx u + hy v + hz w),  h = hemi_sets[set][depth-1][i]
    //   Glossy     (brdf.rs:57-69): w = r,  u = normalize((0.00424, 1, 0.00764) x w), v = u x w,
    //                               wi = hx u + hy v + hz w (mirrored in the frame if below the surface),
    //                               h = to_unit_hemi(pixel sample, exponent)
    // i.e. b1 = normalize(a x w), b2 = b1 x w with (u, v) = (b2, b1) resp. (b1, b2).  Lanes of either kind run
    // the shared part together; the weight f (n.wi)/pdf is the closed form (FAST note at the top).
    V3 wi;
    double scale = 1.0;
    const bool matte = kind == kMatMatte;
    FLUX_CENSUS(P, 6 + cz);  // the lobe code: every lane whose path continues
    if (UNI && !TRIS && LF != kLobeOff && matte && lf.on) {
        LobeFrameU f = lf;
        if (LF == kLobeLate) {
            const LobeFrameScalar F = (LobeFrameScalar)(reinterpret_cast<uintptr_t>(P.lobe_frame) + (uint32_t)hit * (uint32_t)kLobeFrameBytes);
            f.b1x = F[0]; f.b1y = F[1]; f.b1z = F[2];
            f.b2x = F[3]; f.b2y = F[4]; f.b2z = F[5];
        }
        FLUX_CENSUS(P, 7 + cz);
        FLUX_CENSUS(P, 18);
        if (STATS) st.c[2]++;
        const char *hbase = reinterpret_cast<const char *>(set_rows_of(P, set).hemi);
        const uint32_t hoff = ((uint32_t)(p.depth - 1) * (uint32_t)P.nsamp + i) * 32u;
        const double2 hxy = gather_global_d2(hbase, hoff);
        const double hz = gather_global<double>(hbase, hoff + 16u);
        // q = hy b1 + hx b2, wi = hz n + q
        const double qx = __builtin_fma(f.b2x, hxy.x, f.b1x * hxy.y);
        const double qy = __builtin_fma(f.b2y, hxy.x, f.b1y * hxy.y);
        const double qz = __builtin_fma(f.b2z, hxy.x, f.b1z * hxy.y);
        V3 wt = mk(__builtin_fma(f.nx, hz, qx), __builtin_fma(f.ny, hz, qy), __builtin_fma(f.nz, hz, qz));
        if (p_glossy_long && !unit_n) wt = normalize(wt);  // (a stored normal that is not unit: see below)
        p.self = -1;  // (not a convex sphere)
        advance_path<FIRST>(p, pt, wt, fr, fg, fb, 1.0);
        return;
    }
    // The dielectric branch exists only in the FAST copy that serves scenes with a dielectric (FLUX_DIEL: render.hip's third
    // inclusion of this file, chosen by RenderParams::has_diel) and, there, outside TYP (the launch never picks it for such a scene).
    // The copy every other scene runs is compiled without it, so its code -- and, under contract(fast), every fusion decision of the
    // lobe code -- is the one it had before the material existed.
#if FLUX_DIEL
    if (!TYP && kind == kMatDielectric) {  // extension: DESIGN.md §5c
        // u: the hemi sample the Matte lobe reads at this depth (hemi_sets' z), addressed as there
        const char *hbase = !TRIS ? reinterpret_cast<const char *>(set_rows_of(P, set).hemi)
                                  : reinterpret_cast<const char *>(P.hemi + (size_t)set * P.max_depth * P.nsamp * 4);
        const double u = gather_global<double>(hbase, ((uint32_t)(p.depth - 1) * P.nsamp + i) * 32u + 16u);
        if (dielectric_dir(n, d, m_inv_e1, u, wi)) {  // reflected: weight 1; transmitted: transmit_color, (fr, fg, fb) as loaded
            if (STATS) st.c[10]++;
            fr = fg = fb = 1.0;
        } else {
            if (STATS) st.c[11]++;
        }
    } else
#endif
    {
        V3 w = n;
        if (!matte) {  // Reflective::path_shade materials.rs:56-72: r = -wo + n (n.wo) 2, wo = -d
            const double ndotwo = -dot(n, d);
            w = mk(d.x + n.x * ndotwo * 2.0, d.y + n.y * ndotwo * 2.0, d.z + n.z * ndotwo * 2.0);
        }
        if (kind == kMatReflective) {  // PerfectSpecular::sample_f brdf.rs:38-46
            if (STATS) st.c[4]++;
            wi = w;
        } else {
            double hx, hy, hz;
            double c1u = 0.0, c2u = 0.0;  // UNI: (c1, c2) named where the branch knows the material
            if (matte) {
                FLUX_CENSUS(P, 7 + cz);
                if (STATS) st.c[2]++;
                const size_t N = P.nsamp;
                // wave-uniform base (this pixel's set) + 32-bit per-lane byte offset -> saddr + voffset addressing
                // analytic kernels: the set's rows from the context's DevSetRows record, one scalar load instead of a 64-bit multiply-add chain
                // (a scalar instruction costs the issue-bound loop a third of a VALU instruction); the mesh kernels keep the arithmetic
                // (their shading step is rare and the extra dependent load measured +0.5 % there)
                const char *hbase = !TRIS ? reinterpret_cast<const char *>(set_rows_of(P, set).hemi)
                                                             : reinterpret_cast<const char *>(P.hemi + (size_t)set * P.max_depth * N * 4);
                const uint32_t hoff = ((uint32_t)(p.depth - 1) * (uint32_t)N + i) * 32u;
                const double2 hxy = gather_global_d2(hbase, hoff);
                hx = hxy.x;
                hy = hxy.y;
                hz = gather_global<double>(hbase, hoff + 16u);
                c1u = hy;
                c2u = hx;
                if (TRIS && is_tri) scale = 1.0 / kInvPi;  // (n.wi) / ((n.wi) INV_PI); an analytic shape's record holds the product already
            } else {
                FLUX_CENSUS(P, 8 + cz);
                if (STATS) st.c[3]++;
                // to_unit_hemi(pixel sample, exponent) (brdf.rs:64, lib.rs:133-142) with its sample-only factors read
                // from the table (RenderParams::gloss): cos_theta = (1-y)^(1/(e+1)) = exp2(log2(1-y)/(e+1))
                const char *gbase = !TRIS ? reinterpret_cast<const char *>(set_rows_of(P, set).gloss)
                                                             : reinterpret_cast<const char *>(P.gloss + (size_t)set * P.nsamp * 4);
                const double2 cs = gather_global_d2(gbase, i * 32u);
                double cos_theta, sin_theta;
                // ... and, in the analytic kernels, (cos theta, sin theta) themselves where the context tabulated them for the scene's
                // exponents (RenderParams::glossx: the fill applies the operations below, bit for bit): one 16-B gather at the sample's
                // entry for the record's exponent.  TYP: the launch plan picks it only with the table.  Elsewhere: the launch's flag.
                if (!TRIS && (TYP || P.gx_stride != 0)) {
                    const uint32_t xoff = __umul24(i, (uint32_t)P.gx_stride) + (uint32_t)gather_global<int32_t>(P.gx_off, (uint32_t)hit << 2);
                    const double2 csx = gather_global_d2(set_rows_of(P, set).glossx, xoff);
                    cos_theta = csx.x;
                    sin_theta = csx.y;
                } else {
                    cos_theta = fastmath::fexp2_tab(m_inv_e1 * gather_global<double>(gbase, i * 32u + 16u), P.exp2c);   // 1 - y > 0 for every sample (y < 1)
                    sin_theta = fastmath::fsqrt(1.0 - cos_theta * cos_theta);  // (contracted to ONE fused multiply-add: the fill spells it out)
                }
                hx = sin_theta * cs.x;
                hy = sin_theta * cs.y;
                hz = cos_theta;
                c1u = hx;
                c2u = hy;
            }
            const V3 b1 = normalize(cross(mk(ax, 1.0, az), w));
            const V3 b2 = cross(b1, w);
            const double c1 = UNI ? c1u : (matte ? hy : hx), c2 = UNI ? c2u : (matte ? hx : hy);
            const V3 q = mk(c1 * b1.x + c2 * b2.x, c1 * b1.y + c2 * b2.y, c1 * b1.z + c2 * b2.z);
            const V3 hw = mk(hz * w.x, hz * w.y, hz * w.z);
            const V3 wi0 = mk(q.x + hw.x, q.y + hw.y, q.z + hw.z);
            if (matte) {
                // brdf.rs:26 normalises wi; with a unit normal the frame (b2, b1, w) is orthonormal and h is a unit vector, so
                // |wi0| = 1 to a few ulp already and the division changes nothing above rounding (as in to_unit_hemi): it is
                // kept for the hits whose normal is NOT unit (a plane stored with a non-unit normal)
                wi = wi0;
                if (UNI) {
                    if (p_glossy_long && !unit_n) wi = normalize(wi0);
                } else if (p_glossy_long) {  // the scene's flag (abi.hip): a scalar compare instead of a vote of the wave on `!unit_n`
                    const V3 wn = normalize(wi0);
                    wi = unit_n ? wi0 : wn;
                }
            } else {  // brdf.rs:67-69: below the surface -> (-hx) u - hy v + hz w
                const bool below = dot(n, wi0) < 0.0;
                wi = wi0;
                if (ballot64(below) != 0ull)  // (the mirrored direction and its six selects only in a wave that has such a lane)
                    wi = mk(below ? hw.x - q.x : wi0.x, below ? hw.y - q.y : wi0.y, below ? hw.z - q.z : wi0.z);
                // The closed-form weight cs ks is the long form's value whenever the lobe (r.wi)^e is finite and non-zero.
                // r.wi = hz |r|^2 and |r| = |d| for a unit normal, so it can only under- or overflow after a specular bounce off
                // a NON-unit normal.  A scene that has one (a plane stored with a non-unit normal: P.glossy_long, uniform for the
                // whole launch) takes the reference's long form (brdf.rs:73-76, materials.rs:69-70) for every glossy bounce and
                // so gets its NaN (0 * inf) or subnormal-degraded weights; every other scene skips this with one scalar branch.
                if (p_glossy_long) {
                    const double rdotwi = dot(w, wi), ndotwi = dot(n, wi);
                    const DevMaterial &Ml = P.mats[is_tri ? P.tris[slot].mat : P.frec[hit].orig_id];  // (a shape's material has the shape's index)
                    const double e = Ml.exponent;
                    const int parity = Ml.exp_parity;
                    // powf: negative base -> +|x|^e for an even integral e, -|x|^e for an odd one, NaN otherwise
                    double lobe = fastmath::fpow_pos(fabs(rdotwi), e);
                    if (e == 0.0) lobe = 1.0;
                    if (rdotwi < 0.0) lobe = parity == 1 ? lobe : (parity == 2 ? -lobe : __builtin_nan(""));
                    if (rdotwi != rdotwi) lobe = rdotwi;
                    const double pdf = lobe * ndotwi;
                    fr *= lobe;  // f = cs ks lobe (brdf.rs:75)
                    fg *= lobe;
                    fb *= lobe;
                    scale = ndotwi / pdf;
                }
            }
        }
    }
    // A mirrored direction r = d + 2 (n.wo) n inherits |d|, so over a chain of specular / glossy bounces the length would drift
    // from 1 by a few ulp per bounce, and scan_shapes_fast takes it as unit (unit_dirs): one Newton step of the normalisation,
    // wi (3/2 - |wi|^2 / 2), exact to the square of the deviation, keeps every such direction within an ulp of unit length.
    // (A Matte bounce builds its direction afresh around the unit normal: nothing accumulates there.)
    // (the factor is selected per lane -- exactly 1 for a Matte bounce --, not the three products: two selects instead of six)
    if (UNI) {
        if (p_unit_dirs && !matte) {  // (Matte: x 1.0 is x)
            double ww = dot(wi, wi);
            asm("" : "+v"(ww));  // (keeps the branch: the optimiser would run the step for every wave and select its result)
            const double ss = __builtin_fma(-0.5, ww, 1.5);
            wi = mk(wi.x * ss, wi.y * ss, wi.z * ss);
        }
    } else if (p_unit_dirs) {
        const double ss = matte ? 1.0 : __builtin_fma(-0.5, dot(wi, wi), 1.5);
        wi = mk(wi.x * ss, wi.y * ss, wi.z * ss);
    }
    // the child leaves a convex sphere outwards from a hit at most 1e3 away: it cannot hit that sphere again (scan_shapes_fast)
    // (t < 1e3 on the high word: 1000.0 is 0x408f4000'00000000, so for every double -- negative, infinite, NaN -- the signed compare of
    // the high words decides as the f64 compare does, and its 32-bit literal sits in the instruction where the f64 one took two scalar moves)
    if (UNI) {
        p.self = -1;
        if (p_self_skip && convex) p.self = (__double2hiint(t) < 0x408f4000 && dot(n, wi) >= 0.0) ? hit : -1;
    } else {
        p.self = (p_self_skip && convex && __double2hiint(t) < 0x408f4000 && dot(n, wi) >= 0.0) ? hit : -1;
    }
    advance_path<FIRST>(p, pt, wi, fr, fg, fb, scale);
}

// The fields of an analytic shape's hit (shapes.rs:140-146,191-197) from its record: gathered per lane, one batch of independent
// loads (DevHitRec) instead of shape -> kind -> fields -> material chains.  Returns the shape's material index.  One copy, shared by
// the shading step (shade_hit_fast) and the split kernel's bounce of a parked hit (bounce_parked_hit), so that both form the normal
// from the same operands with the same operations.
// UNI: `hit` is wave-uniform, so the record is too: ONE read of P.frec[hit] through the scalar cache (the records are constant for
// the kernel's lifetime: the constant address space says so) instead of a 96-byte gather per lane, and a scalar branch on the shape's
// kind instead of the select -- the sphere's normal is formed only for a sphere.  lf (LF != kLobeOff): whether the uniform step takes
// the record's lobe frame from the table and, with kLobeEarly, the entry itself.
typedef const __attribute__((address_space(4))) DevHitRec *HitRecScalar;
template <bool LDS_SCENE, bool UNI = false, int LF = kLobeOff>
__device__ __forceinline__ int analytic_hit_fields(const RenderParams &P, const Ray &r, int hit, double t, const char *frec_lds, V3 &n,
                                                   int &kind, bool &unit_n, bool &convex, double &fr, double &fg, double &fb,
                                                   double &m_inv_e1, double &ax, double &az, LobeFrameU *lf = nullptr) {
    (void)frec_lds;
    if (UNI) {
        const HitRecScalar Ru = (HitRecScalar)(reinterpret_cast<uintptr_t>(P.frec) + (uint32_t)hit * (uint32_t)sizeof(DevHitRec));
        if (LF != kLobeOff) {
            const bool tab = P.lobe_frame != nullptr;
            if (LF == kLobeEarly) {
                // (a context without the table: the same six loads from the record's own bytes, which are there to be read, and `on`
                // says that they mean nothing -- an address selected with two scalar instructions, where a branch around the loads
                // would put a wait of its own between them and the record's)
                const LobeFrameScalar F = (LobeFrameScalar)(tab ? reinterpret_cast<uintptr_t>(P.lobe_frame) + (uint32_t)hit * (uint32_t)kLobeFrameBytes
                                                                : reinterpret_cast<uintptr_t>(Ru));
                lf->b1x = F[0]; lf->b1y = F[1]; lf->b1z = F[2];
                lf->b2x = F[3]; lf->b2y = F[4]; lf->b2z = F[5];
            }
            lf->nx = Ru->cx; lf->ny = Ru->cy; lf->nz = Ru->cz;
            lf->on = tab && Ru->shape_kind != kShapeSphere;
        }
        kind = Ru->mat_kind;
        unit_n = Ru->unit_normal != 0;
        fr = Ru->fr; fg = Ru->fg; fb = Ru->fb; m_inv_e1 = Ru->inv_e1;
        ax = Ru->ax; az = Ru->az;
        const double cx = Ru->cx, cy = Ru->cy, cz = Ru->cz, inv_rad = Ru->inv_rad;
        if (Ru->shape_kind == kShapeSphere) {
            n = mk(((r.ox - cx) + t * r.dx) * inv_rad, ((r.oy - cy) + t * r.dy) * inv_rad, ((r.oz - cz) + t * r.dz) * inv_rad);
            convex = inv_rad > 0.0;
        } else {
            n = mk(cx, cy, cz);
            convex = false;
        }
        return Ru->orig_id;
    }
    const DevHitRec R = *reinterpret_cast<const DevHitRec *>((LDS_SCENE ? frec_lds : reinterpret_cast<const char *>(P.frec)) +
                                                              (uint32_t)hit * (uint32_t)sizeof(DevHitRec));
    kind = R.mat_kind;
    unit_n = R.unit_normal != 0;
    fr = R.fr; fg = R.fg; fb = R.fb; m_inv_e1 = R.inv_e1;
    ax = R.ax; az = R.az;
    // sphere: (temp + t d) * invert_val / radius with invert_val/radius in one rounding; plane: stored normal
    const V3 ns = mk(((r.ox - R.cx) + t * r.dx) * R.inv_rad, ((r.oy - R.cy) + t * r.dy) * R.inv_rad,
                     ((r.oz - R.cz) + t * r.dz) * R.inv_rad);
    const bool sph = R.shape_kind == kShapeSphere;
    n = mk(sph ? ns.x : R.cx, sph ? ns.y : R.cy, sph ? ns.z : R.cz);
    convex = sph && R.inv_rad > 0.0;
    return R.orig_id;  // a shape's material has the shape's index
}

// FAST, in two phases.  Phase 1, every lane of the shading step: what was hit, and the two ways a path ENDS (a miss, an emitter)
// as values.  Phase 2, the lanes that bounce: the lobe code and the ONLY update of the loop-carried path state, under one plain
// `if` that follows the join of phase 1.  Written with early returns (as the reference's match arms suggest, and as round 1-3 had
// it) the bounce is one of three ways out of the function, the structuriser turns that into flow blocks, and the value of the
// state for the next pass gets defined -- as a copy of the old one -- where the ways part, i.e. while the old one is still
// needed: two register sets for the state and ~14 v_mov_b64 into and out of them on every way through, every pass.  The empty asm
// keeps the compiler from threading `bounce` back into phase 1 (it is 1 on exactly one way into the join).
// BOUNCE = false (the split kernel's phase B with its hit queue): phase 1 only -- the hit is classified, a continuing path's state is
// left as it was and its bounce runs later from the parked hit (bounce_parked_hit).
// FACING (with BOUNCE = false): `facing` is the scan's word on which side of the winner the ray met (scan_shapes_fast, sphere_facing).
// UNI (analytic shapes): `hit` is wave-uniform (shade_primary_hits).  The three ways out are then scalar branches, so the bounce runs where the
// hit is classified: no join, and none of the defaults the join defines for the ways that do not bounce.
template <bool STATS, bool TRIS, bool LDS_SCENE = false, bool TYP = false, bool FIRST = false, bool BOUNCE = true, bool FACING = false,
          bool UNI = false, int LF = kLobeOff>
__device__ __forceinline__ bool shade_hit_fast(const RenderParams &P, Path &p, uint32_t set, uint32_t i, int hit, int slot, double t,
                                               double &Lr, double &Lg, double &Lb, Stats &st, int cz, const char *frec_lds = nullptr,
                                               int facing = 0) {
    (void)frec_lds;  // LDS_SCENE: the block's LDS copy of the hit records
    (void)facing;
    (void)cz;  // census builds: section offset of the caller (split kernel: 0 = phase B, 3 = phase A)
    int bounce = 0;
    const bool is_tri = TRIS && slot >= 0;
    const V3 d = mk(p.r.dx, p.r.dy, p.r.dz);
    const V3 pt = mk(p.r.ox + t * d.x, p.r.oy + t * d.y, p.r.oz + t * d.z);
    V3 n = mk(0.0, 0.0, 1.0);
    int kind = kMatEmissive;
    bool unit_n = true;   // triangles store normalize(e1 x e2)
    bool convex = false;  // a sphere hit whose stored normal points outwards (not `invert`)
    double fr = 0.0, fg = 0.0, fb = 0.0, m_inv_e1 = 0.0, ax = 0.0, az = 0.0;
    LobeFrameU lf;  // UNI: the record's lobe frame, where the context tabulated it
    if (hit < 0) {  // scene.rs:168
        Lr = P.bgr;
        Lg = P.bgg;
        Lb = P.bgb;
        if (STATS) st.c[6]++;
    } else {
        // Hit fields of the winning shape (shapes.rs:140-146,191-197): gathered per lane
        // one batch of independent loads (DevHitRec) instead of shape -> kind -> fields -> material chains
        if (is_tri) {
            const DevTri &T = P.tris[slot];
            const DevMaterial &Mt = P.mats[T.mat];
            p.mat = T.mat;
            n = tri_shading_normal(P, p.r, slot, reinterpret_cast<const char *>(P.mats), (uint32_t)sizeof(DevMaterial), T.mat, fr, fg, fb);
            kind = Mt.kind;
            m_inv_e1 = Mt.inv_e1;
            ax = kind == kMatMatte ? 0.0034 : 0.00424;  // brdf.rs:22 / brdf.rs:58
            az = kind == kMatMatte ? 0.0071 : 0.00764;
        } else {
            p.mat = analytic_hit_fields<LDS_SCENE, UNI, UNI ? LF : kLobeOff>(P, p.r, hit, t, frec_lds, n, kind, unit_n, convex, fr, fg, fb, m_inv_e1,
                                                                             ax, az, &lf);
        }
        if (kind == kMatEmissive) {  // materials.rs:41-50
            if (STATS) st.c[5]++;
            bool front;
            // FACING: the normal has no other consumer here, so where the scan knows the side of every Emissive hit of the wave the
            // test is two integer operations on the record's inv_rad -- no record reads for the centre, no point, no normal, no dot
            // product.  One vote; a wave with an Emissive lane the scan does not vouch for (a plane, a disk, a grazing hit, a pass
            // outside the guards) computes the test for all of them as ever.
            if (FACING && ballot64(!facing_known(facing)) == 0ull) {
                const DevHitRec &R = *reinterpret_cast<const DevHitRec *>(frec_lds + (uint32_t)hit * (uint32_t)sizeof(DevHitRec));
                front = facing_front(facing, reinterpret_cast<const int *>(&R.inv_rad)[1]);
            } else {
                front = ((n.x * -1.0) * d.x + (n.y * -1.0) * d.y + (n.z * -1.0) * d.z) > 0.0;
            }
            Lr = fr;
            Lg = fg;
            Lb = fb;
            // an emitter seen from behind is black: rare (the inside of a convex light, the outside of an environment), so the six
            // selects run only in a wave that has such a lane (a vote on the compare: scalar).  (Handing (fr, fg, fb) back as L for
            // all three ways out -- no copies at all -- was measured: 0.9 % SLOWER, profiles/r06_experiments/ab_m1_m3_r06g.log.)
            if (ballot64(!front) != 0ull) {
                Lr = front ? fr : 0.0;
                Lg = front ? fg : 0.0;
                Lb = front ? fb : 0.0;
            }
        } else {
            if (UNI) {
                if (BOUNCE) fast_bounce<STATS, TRIS, TYP, FIRST, true, LF>(P, p, set, i, hit, slot, t, n, d, pt, kind, fr, fg, fb, m_inv_e1, ax,
                                                                           az, unit_n, convex, is_tri, st, cz, lf);
                return true;
            }
            bounce = 1;
        }
    }
    if (UNI) return false;
    asm("" : "+v"(bounce));
    if (BOUNCE && bounce) {
        fast_bounce<STATS, TRIS, TYP, FIRST>(P, p, set, i, hit, slot, t, n, d, pt, kind, fr, fg, fb, m_inv_e1, ax, az, unit_n, convex, is_tri, st,
                                            cz);
    }
    return bounce != 0;
}

// The other half of shade_hit_fast for a hit the split kernel parked in its hit queue (an analytic shape, records in LDS): the
// bounce from (o, d, t, hit) -- p.r holds the segment (o, d) --, with the operands and operations of the shading step that
// classified it (analytic_hit_fields, pt = o + t d, fast_bounce): the path's next ray is bit for bit the one the step would have made.
template <bool STATS, bool TYP>
__device__ __forceinline__ void bounce_parked_hit(const RenderParams &P, Path &p, uint32_t set, uint32_t i, int hit, double t, Stats &st,
                                                  int cz, const char *frec_lds) {
    const V3 d = mk(p.r.dx, p.r.dy, p.r.dz);
    const V3 pt = mk(p.r.ox + t * d.x, p.r.oy + t * d.y, p.r.oz + t * d.z);
    V3 n;
    int kind;
    bool unit_n, convex;
    double fr, fg, fb, m_inv_e1, ax, az;
    p.mat = analytic_hit_fields<true>(P, p.r, hit, t, frec_lds, n, kind, unit_n, convex, fr, fg, fb, m_inv_e1, ax, az);
    fast_bounce<STATS, false, TYP, false>(P, p, set, i, hit, -1, t, n, d, pt, kind, fr, fg, fb, m_inv_e1, ax, az, unit_n, convex, false, st, cz);
}
#endif

// The part of Scene::shade after Scene::hit (scene.rs:167-171): `hit` / `slot` / `t` as returned by
// scene_hit.  Returns true if the path continues (`p.r` holds the child ray, depth advanced).
template <bool STATS, bool TRIS, bool TWO_PHASE = false, bool LDS_SCENE = false, bool TYP = false>
__device__ __forceinline__ bool shade_hit(const RenderParams &P, Path &p, uint32_t set, uint32_t i, int hit,
                                          int slot, double t, double *stk, int stk_stride, double &Lr,
                                          double &Lg, double &Lb, Stats &st, int cz = 0, const char *frec_lds = nullptr,
                                          const char *mats_lds = nullptr) {
    (void)cz;  // census builds: section offset of the caller (split kernel: 0 = phase B, 3 = phase A)
    (void)frec_lds;  // LDS_SCENE (render_bvh4_kernel): the block's LDS copies of the hit records and the materials
    (void)mats_lds;
#if FLUX_FAST
    // (per caller: the split kernel gains from it; render_bvh4_kernel -- 91 registers, none spilled -- would spill six with it)
    if (TWO_PHASE) return shade_hit_fast<STATS, TRIS>(P, p, set, i, hit, slot, t, Lr, Lg, Lb, st, cz);
#endif
    if (hit < 0) {  // scene.rs:168
        Lr = P.bgr;
        Lg = P.bgg;
        Lb = P.bgb;
        if (STATS) st.c[6]++;
        return false;
    }
    // Hit fields of the winning shape (shapes.rs:140-146,191-197): gathered per lane
    const bool is_tri = TRIS && slot >= 0;
    const V3 d = mk(p.r.dx, p.r.dy, p.r.dz);
    const V3 pt = mk(p.r.ox + t * d.x, p.r.oy + t * d.y, p.r.oz + t * d.z);
    V3 n;
#if FLUX_FAST
    // one batch of independent loads (DevHitRec) instead of shape -> kind -> fields -> material chains
    int kind;
    bool unit_n = true;  // triangles store normalize(e1 x e2)
    bool convex = false;  // a sphere hit whose stored normal points outwards (not `invert`)
    double fr, fg, fb, m_inv_e1, ax, az;
    if (is_tri) {
        const DevTri &T = P.tris[slot];
        const DevMaterial &Mt = LDS_SCENE ? *reinterpret_cast<const DevMaterial *>(mats_lds + (uint32_t)T.mat * (uint32_t)sizeof(DevMaterial))
                                          : P.mats[T.mat];
        p.mat = T.mat;
        n = tri_shading_normal(P, p.r, slot, LDS_SCENE ? mats_lds : reinterpret_cast<const char *>(P.mats), (uint32_t)sizeof(DevMaterial),
                               T.mat, fr, fg, fb);
        kind = Mt.kind;
        m_inv_e1 = Mt.inv_e1;
        ax = kind == kMatMatte ? 0.0034 : 0.00424;  // brdf.rs:22 / brdf.rs:58
        az = kind == kMatMatte ? 0.0071 : 0.00764;
    } else {
        const DevHitRec R = *reinterpret_cast<const DevHitRec *>((LDS_SCENE ? frec_lds : reinterpret_cast<const char *>(P.frec)) +
                                                                  (uint32_t)hit * (uint32_t)sizeof(DevHitRec));
        kind = R.mat_kind;
        p.mat = R.orig_id;  // a shape's material has the shape's index
        unit_n = R.unit_normal != 0;
        fr = R.fr; fg = R.fg; fb = R.fb; m_inv_e1 = R.inv_e1;
        ax = R.ax; az = R.az;
        // sphere: (temp + t d) * invert_val / radius with invert_val/radius in one rounding; plane: stored normal
        const V3 ns = mk(((p.r.ox - R.cx) + t * d.x) * R.inv_rad, ((p.r.oy - R.cy) + t * d.y) * R.inv_rad,
                         ((p.r.oz - R.cz) + t * d.z) * R.inv_rad);
        const bool sph = R.shape_kind == kShapeSphere;
        n = mk(sph ? ns.x : R.cx, sph ? ns.y : R.cy, sph ? ns.z : R.cz);
        convex = sph && R.inv_rad > 0.0;
    }
    if (kind == kMatEmissive) {  // materials.rs:41-50
        if (STATS) st.c[5]++;
        const bool front = ((n.x * -1.0) * d.x + (n.y * -1.0) * d.y + (n.z * -1.0) * d.z) > 0.0;
        Lr = front ? fr : 0.0;
        Lg = front ? fg : 0.0;
        Lb = front ? fb : 0.0;
        return false;
    }
#else
    const DevShape *S = P.shapes + (is_tri ? 0 : hit);
    const DevMaterial *M = P.mats + (is_tri ? P.tris[slot].mat : hit);
    double tfr = 0.0, tfg = 0.0, tfb = 0.0;  // a triangle's triple, times its colour factor where it has one (DESIGN.md section 5k)
    if (is_tri) {
        n = tri_shading_normal(P, p.r, slot, reinterpret_cast<const char *>(P.mats), (uint32_t)sizeof(DevMaterial), P.tris[slot].mat, tfr,
                               tfg, tfb);
    } else if (S->kind == kShapeSphere) {
        const double inv = S->inv, rad = S->radius;
        n = mk(((p.r.ox - S->px) + t * d.x) * inv / rad, ((p.r.oy - S->py) + t * d.y) * inv / rad,
               ((p.r.oz - S->pz) + t * d.z) * inv / rad);
    } else if (S->kind == kShapeBox) {
        // the face scene_hit found (slot = -2 - face): its outward unit axis, negated for `invert` -- the bits of FAST's face record
        const int face = -2 - slot;
        const double v = ((face & 1) ? 1.0 : -1.0) * S->inv;
        n = mk(face < 2 ? v : 0.0, (face >> 1) == 1 ? v : 0.0, face >= 4 ? v : 0.0);
    } else {
        n = mk(S->c0x, S->c0y, S->c0z);
    }
    const int kind = M->kind;
    if (kind == kMatEmissive) {  // materials.rs:41-50
        if (STATS) st.c[5]++;
        const bool front = ((n.x * -1.0) * d.x + (n.y * -1.0) * d.y + (n.z * -1.0) * d.z) > 0.0;
        Lr = front ? (is_tri ? tfr : M->fr) : 0.0;
        Lg = front ? (is_tri ? tfg : M->fg) : 0.0;
        Lb = front ? (is_tri ? tfb : M->fb) : 0.0;
        return false;
    }
    double fr = is_tri ? tfr : M->fr, fg = is_tri ? tfg : M->fg, fb = is_tri ? tfb : M->fb;
    const double m_exponent = M->exponent, m_inv_e1 = M->inv_e1;
#endif
#if FLUX_FAST
    fast_bounce<STATS, TRIS, TYP>(P, p, set, i, hit, slot, t, n, d, pt, kind, fr, fg, fb, m_inv_e1, ax, az, unit_n, convex, is_tri, st, cz);
    return true;
#else
    // STRICT.  The two sampled lobes share ONE frame construction (round 5), as in FAST -- and here bit for bit:
    //   Lambertian (brdf.rs:22-27): w = n,  v = normalize((0.0034, 1, 0.0071) x w),  u = v x w,
    //                               wi = normalize((hx u + hy v) + hz w),  h = hemi_sets[set][depth-1][i]
    //   Glossy     (brdf.rs:57-69): w = r,  u = normalize((0.00424, 1, 0.00764) x w), v = u x w,
    //                               wi0 = (u hx + v hy) + w hz, mirrored in the frame if below the surface
    // i.e. b1 = normalize(a x w), b2 = b1 x w with (u, v) = (b2, b1) resp. (b1, b2): the SAME operations on per-lane operands
    // (the constants of `a` and the roles of hx / hy are selected per lane), and hx u + hy v = hy b1 + hx b2 resp.
    // u hx + v hy = hx b1 + hy b2 are the same IEEE sums whichever term comes first.  Written as two blocks -- as the reference's
    // two impls suggest and as rounds 1-4 had it -- a wave that holds Matte AND Glossy lanes ran cross + normalize (a square root and
    // three IEEE divisions) + cross twice, each under a partial mask.  Frames and statistics equal the two-block form's bit for bit
    // (checked against a build of the old form: profiles/r05_experiments/strict_filter_check3.log).
    V3 wi;
    double scale;  // (n . wi) / pdf
    const bool matte = kind == kMatMatte;
    // (STRICT: one copy for every scene, the branch behind the scene's uniform flag -- without contraction the code around it computes
    // the same bits whatever shape the branch gives the control flow)
    if (P.has_diel != 0 && kind == kMatDielectric) {  // extension: DESIGN.md §5c -- the entry (1, 1, 1, 1) or (transmit_color, 1)
        const double *hp = P.hemi + (((size_t)set * P.max_depth + (p.depth - 1)) * P.nsamp + i) * 4;
        if (dielectric_dir(n, d, m_inv_e1, hp[2], wi)) {
            if (STATS) st.c[10]++;
            fr = fg = fb = 1.0;
        } else {
            if (STATS) st.c[11]++;
        }
        scale = 1.0;
    } else {
        V3 w = n;
        if (!matte) {
            // Reflective::path_shade materials.rs:56-72; wo = -d, so -wo = d exactly
            const V3 wo = mk(d.x * -1.0, d.y * -1.0, d.z * -1.0);
            const double ndotwo = dot(n, wo);
            w = mk(-wo.x + n.x * ndotwo * 2.0, -wo.y + n.y * ndotwo * 2.0, -wo.z + n.z * ndotwo * 2.0);  // r
        }
        if (kind == kMatReflective) {  // PerfectSpecular::sample_f brdf.rs:38-46
            if (STATS) st.c[4]++;
            wi = w;
            const double pdf = dot(n, wi);
            scale = dot(n, wi) / pdf;
        } else {
            double hx, hy, hz;
            if (matte) {  // materials.rs:18-34 + Lambertian::sample_f brdf.rs:19-31
                if (STATS) st.c[2]++;
                const size_t N = P.nsamp;
                const double *hp = P.hemi + (((size_t)set * P.max_depth + (p.depth - 1)) * N + i) * 4;
                const double2 hxy = *reinterpret_cast<const double2 *>(hp);
                hx = hxy.x;
                hy = hxy.y;
                hz = hp[2];
            } else {  // GlossySpecular::sample_f brdf.rs:54-79
                if (STATS) st.c[3]++;
                FLUX_STAGE();
                const V3 h = to_unit_hemi(p.sq, m_inv_e1);
                FLUX_STAGE();
                hx = h.x;
                hy = h.y;
                hz = h.z;
            }
            const double ax = matte ? 0.0034 : 0.00424, az = matte ? 0.0071 : 0.00764;
            const V3 b1 = normalize(cross(mk(ax, 1.0, az), w));
            const V3 b2 = cross(b1, w);
            const double c1 = matte ? hy : hx, c2 = matte ? hx : hy;  // the coefficients of b1 and b2
            const V3 q = mk(c1 * b1.x + c2 * b2.x, c1 * b1.y + c2 * b2.y, c1 * b1.z + c2 * b2.z);
            const V3 hw = mk(hz * w.x, hz * w.y, hz * w.z);
            const V3 wi0 = mk(q.x + hw.x, q.y + hw.y, q.z + hw.z);
            if (matte) {
                wi = normalize(wi0);  // brdf.rs:26
                const double ndotwi = dot(n, wi);
                const double pdf = ndotwi * kInvPi;
                scale = ndotwi / pdf;
            } else {
                // brdf.rs:67-69: below the surface -> (u (-hx) - v hy) + w hz = (-q) + hw (a negated sum is the sum of the negated
                // terms, exactly)
                const bool below = dot(n, wi0) < 0.0;
                wi = mk(below ? hw.x - q.x : wi0.x, below ? hw.y - q.y : wi0.y, below ? hw.z - q.z : wi0.z);
                const double lobe = pow(dot(w, wi), m_exponent);
                const double pdf = lobe * dot(n, wi);
                fr = fr * lobe;
                fg = fg * lobe;
                fb = fb * lobe;
                scale = dot(n, wi) / pdf;
            }
        }
    }
    // record (f, s); child ray starts at the hit point (materials.rs:26-29,65-68)
    double *e = stk + (size_t)p.nb * 4 * stk_stride;
    e[0] = fr;
    e[stk_stride] = fg;
    e[2 * stk_stride] = fb;
    e[3 * stk_stride] = scale;
    p.nb++;
    p.depth++;
    p.r.ox = pt.x;
    p.r.oy = pt.y;
    p.r.oz = pt.z;
    p.r.dx = wi.x;
    p.r.dy = wi.y;
    p.r.dz = wi.z;
    return true;
#endif
}

// One Scene::shade level (scene.rs:162-172) for a live lane.  Returns true if
// the path continues (a bounce was recorded and `p.r` now holds the child ray);
// otherwise (Lr,Lg,Lb) is the value this level returns.
template <bool STATS, bool TRIS>
__device__ __forceinline__ bool shade_level(const RenderParams &P, Path &p, uint32_t set, uint32_t i,
                                            double *stk, int stk_stride, int *tstack, double &Lr, double &Lg,
                                            double &Lb, Stats &st) {
    if (p.depth > P.max_depth) {  // scene.rs:164-165
        Lr = Lg = Lb = 0.0;
        if (STATS) st.c[7]++;
        return false;
    }
    if (STATS) st.c[1]++;
    double t;
    int slot;
    const int hit = scene_hit<STATS, TRIS>(P, p.r, path_self(p), t, slot, tstack, stk_stride, st);
    return shade_hit<STATS, TRIS>(P, p, set, i, hit, slot, t, stk, stk_stride, Lr, Lg, Lb, st);
}

// Unwind the recursion: L <- (f (*) L) * s from the deepest bounce outward
// (materials.rs:31-33,70-71).  FAST: the same product, already accumulated front to back.
__device__ __forceinline__ void fold_path(const Path &p, const double *stk, int stk_stride, double &Lr,
                                          double &Lg, double &Lb) {
#if FLUX_FAST
    Lr *= p.tr;
    Lg *= p.tg;
    Lb *= p.tb;
#else
    for (int k = p.nb - 1; k >= 0; --k) {
        const double *e = stk + (size_t)k * 4 * stk_stride;
        const double s = e[3 * stk_stride];
        Lr = (e[0] * Lr) * s;
        Lg = (e[stk_stride] * Lg) * s;
        Lb = (e[2 * stk_stride] * Lb) * s;
    }
#endif
}

// The 64 per-lane partial sums of a wave, added in a FIXED tree of six pairings carried out in the VALU (no LDS crossbar:
// __shfl_xor is two ds_bpermute_b32 per double and step, each a round trip through the LDS): lane pairs within a quad
// (quad_perm [1,0,3,2]), quad halves ([2,3,0,1]), the two quads of 8 lanes (row_half_mirror), the two halves of a row of
// 16 (row_mirror), then rows 2j | 2j+1 and the two halves of the wave with gfx950's v_permlane16_swap / v_permlane32_swap
// (two copies of x: one ends up holding the lower partner everywhere, the other the upper).  Every lane ends with the same
// total (a + b and b + a are the same bits), bit-reproducible run to run.
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double x) {
    const int lo = __double2loint(x), hi = __double2hiint(x);
    return __hiloint2double(__builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false),
                            __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ double wave_sum1(double x) {
    x += dpp_f64<0xB1>(x);   // quad_perm [1,0,3,2]
    x += dpp_f64<0x4E>(x);   // quad_perm [2,3,0,1]
    x += dpp_f64<0x141>(x);  // row_half_mirror
    x += dpp_f64<0x140>(x);  // row_mirror
    {
        const unsigned lo = (unsigned)__double2loint(x), hi = (unsigned)__double2hiint(x);
        const auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
        const auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        x = __hiloint2double((int)b[0], (int)a[0]) + __hiloint2double((int)b[1], (int)a[1]);
    }
    {
        const unsigned lo = (unsigned)__double2loint(x), hi = (unsigned)__double2hiint(x);
        const auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
        const auto b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
        x = __hiloint2double((int)b[0], (int)a[0]) + __hiloint2double((int)b[1], (int)a[1]);
    }
    return x;
}
__device__ __forceinline__ void wave_sum3(double sr, double sg, double sb, double &r, double &g, double &b) {
    r = wave_sum1(sr);
    g = wave_sum1(sg);
    b = wave_sum1(sb);
}

// ---- the pieces of a per-pixel pass (aov_kernel, moments_kernel, adaptive_pass_kernel) ----
// (render_static_kernel and finish_pixel below hold the same layout and combine in their own text: seen in a function of their own,
// the layout's two divisions are narrowed to 8 bits by the compiler, and the product kernel's instruction stream is kept as it is)
// The two layouts of a pass whose unit of work -- a pixel, or an entry of a work list -- takes N samples.  From 64 samples on a wave
// is one unit and lane l takes samples l, l + 64, ...; below, 64 / N consecutive units share a wave in groups of N lanes, and the
// 64 % N lanes behind the last group idle (N = 9: seven groups, one idle lane).
struct LaneGroup {
    bool whole_wave;    // N >= 64 (wave-uniform): the wave is one unit
    uint32_t lpp;       // lanes per unit
    uint32_t ppw;       // units per wave
    uint32_t slot;      // the lane's group within the wave (>= ppw: an idle lane)
    uint32_t seg_base;  // the group's first lane
    uint32_t i0;        // the lane within its group: its first sample, and the first channel it stores
    uint64_t wave;      // the wave within the grid
    __device__ __forceinline__ uint64_t unit() const { return wave * ppw + slot; }
    __device__ __forceinline__ bool on(uint64_t units) const { return slot < ppw && unit() < units; }  // not an idle lane, and work left
};
__device__ __forceinline__ LaneGroup lane_group(uint32_t N) {
    LaneGroup G;
    const int tid = threadIdx.x;
    const uint32_t lane = tid & 63;
    G.whole_wave = N >= 64u;
    G.lpp = G.whole_wave ? 64u : N;
    G.ppw = 64u / G.lpp;
    G.wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (tid >> 6);
    G.slot = lane / G.lpp;
    G.seg_base = G.slot * G.lpp;
    G.i0 = lane - G.seg_base;
    return G;
}
// A unit's K totals from its lanes' partial sums, in a fixed order -- a whole wave: wave_sum1's tree; a lane group: in lane order --,
// so what a pass writes is bit-reproducible and does not depend on how rows are grouped into calls.  Every lane of the group ends
// with the totals.
template <int K>
__device__ __forceinline__ void group_totals(const LaneGroup &G, const double (&s)[K], double (&tot)[K]) {
    if (G.whole_wave) {
#pragma unroll
        for (int k = 0; k < K; ++k) tot[k] = wave_sum1(s[k]);
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) tot[k] = 0.0;
        for (uint32_t j = 0; j < G.lpp; ++j) {
            const int src = (int)((G.seg_base + j) & 63u);
#pragma unroll
            for (int k = 0; k < K; ++k) tot[k] += __shfl(s[k], src);
        }
    }
}
// A pass stores a unit's K channels as `for (ch = G.i0; ch < K; ch += G.lpp) o[ch] = pick(ch, v0, v1, ...)` (flux_moments.h): lane j of the
// group writes channels j, j + lpp, ... -- from 8 samples on, eight lanes write a 64-byte line, a double each.

// Sum the per-lane partials of one pixel (a whole wave: wave_sum3's tree; a lane group of a wave that holds several
// pixels: in lane order), then trace.rs:85-87: * 1/n^2, max_to_one, store (leader = first lane of the pixel's group).
__device__ __forceinline__ void finish_pixel(const RenderParams &P, bool lane_on, uint32_t lane,
                                             uint32_t seg_base, uint32_t lpp, uint64_t pixel, double sr,
                                             double sg, double sb) {
    double r = 0.0, g = 0.0, b = 0.0;
    if (lpp == 64u) {  // wave-uniform: the whole wave is one pixel
        wave_sum3(sr, sg, sb, r, g, b);
    } else {
        for (uint32_t k = 0; k < lpp; ++k) {
            const int src = (int)((seg_base + k) & 63u);
            r += __shfl(sr, src);
            g += __shfl(sg, src);
            b += __shfl(sb, src);
        }
    }
    if (lane_on && lane == seg_base) {
        r *= P.pixel_denom;
        g *= P.pixel_denom;
        b *= P.pixel_denom;
        // Color::max_to_one: color.rs:35-44
        const double mx1 = r > g ? r : g;
        const double mx2 = mx1 > b ? mx1 : b;
        if (mx2 > 1.0) {
            const double inv = 1.0 / mx2;
            r *= inv;
            g *= inv;
            b *= inv;
        }
        double *o = P.out + pixel * 3;
        o[0] = r;
        o[1] = g;
        o[2] = b;
    }
}

template <bool STATS>
__device__ __forceinline__ void flush_stats(const RenderParams &P, Stats &st, uint32_t lane) {
    if (!STATS) return;
    for (int c = 0; c < 12; ++c) {
        unsigned v = st.c[c];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0 && v) atomicAdd(P.stats + c, (unsigned long long)v);
    }
}

// LDS per block: strict keeps the (f,s) stack [level][4][thread]; both keep the BVH stack [entry][thread]
__device__ __forceinline__ int *bvh_stack_base(double *lds, const RenderParams &P, int stride) {
#if FLUX_FAST
    return reinterpret_cast<int *>(lds);
#else
    return reinterpret_cast<int *>(lds + (size_t)P.max_depth * 4 * stride);
#endif
}

// wave -> pixel.  Every pixel of a row uses a different sample set (trace.rs:64-69), so the 600 pixels that
// share one set (3 MB of tables) are one per row: in row-major order they run ~800 waves apart and every
// table byte comes from HBM 600 times.  Grouped order instead: wave w -> XCD slot w & 7 (blocks are dealt
// round-robin over the 8 XCDs, MI355X_MICROARCH.md), within it set-major, i.e. the waves resident on one XCD
// work through ONE set's rows at a time and its tables stay in that XCD's L2 (and in the Infinity Cache).
// Placement only affects speed: the pixel computed by a wave does not depend on where it runs.
__device__ __forceinline__ bool map_wave(const RenderParams &P, uint64_t wave, int &lrow, int &col, int &row,
                                         uint32_t &set, uint64_t &out_index) {
    if (P.num_sets == (uint32_t)P.img_w) {
        const uint32_t xcd = (uint32_t)(wave & 7u);
        const uint64_t j = wave >> 3;
        const uint32_t full = (uint32_t)P.set_count >> 3;  // groups of 8 sets: one set per XCD slot at a time
        uint32_t m;                                        // local set index
        if (j < (uint64_t)full * P.num_rows) {
            const uint32_t sidx = (uint32_t)(j / (uint64_t)P.num_rows);
            lrow = (int)(j - (uint64_t)sidx * P.num_rows);
            m = sidx * 8u + xcd;
        } else {
            // the last set_count % 8 sets (a rank's share of 100 sets at G = 8 leaves 4): their rows are dealt over all
            // 8 slots in contiguous runs, so no XCD works through one set more than another
            const uint64_t tail = (uint64_t)((uint32_t)P.set_count & 7u) * P.num_rows;  // pixels left
            const uint64_t per_slot = (tail + 7u) >> 3;
            const uint64_t q = (uint64_t)xcd * per_slot + (j - (uint64_t)full * P.num_rows);
            if (j - (uint64_t)full * P.num_rows >= per_slot || q >= tail) return false;
            const uint32_t sidx = (uint32_t)(q / (uint64_t)P.num_rows);
            lrow = (int)(q - (uint64_t)sidx * P.num_rows);
            m = full * 8u + sidx;
        }
        const uint32_t gset = (uint32_t)P.set_first + m * (uint32_t)P.set_stride;  // global set index: who uses it
        set = (uint32_t)P.slot_first + m * (uint32_t)P.slot_stride;                // where its tables are
        row = P.first_row + lrow * P.row_stride;
        col = P.invperm[(size_t)row * P.num_sets + gset];
        out_index = P.out_by_set ? (uint64_t)lrow * (uint64_t)P.set_count + m : (uint64_t)lrow * P.img_w + col;
        return true;
    }
    if (wave >= (uint64_t)P.num_rows * P.img_w) return false;
    lrow = (int)(wave / P.img_w);
    col = (int)(wave - (uint64_t)lrow * P.img_w);
    row = P.first_row + lrow * P.row_stride;
    set = (uint32_t)P.rowperm[(size_t)row * P.num_sets + col] % P.num_sets;  // trace.rs:68-69
    out_index = (uint64_t)lrow * P.img_w + col;
    return true;
}

// ---------------------------------------------------------------------------
// STATIC variant: lane l of a pixel's lane group traces samples l, l+64, ...;
// a lane idles from the end of its path until the slowest lane of the chunk is done.
// Handles every n (also n*n < 64: 64/(n*n) pixels share a wave).
// ---------------------------------------------------------------------------
template <bool STATS, bool TRIS>
__global__ __launch_bounds__(FLUX_BLOCK_THREADS, FLUX_WPE_WIDE) void render_static_kernel(const RenderParams P) {
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

    int row = 0, col = 0;
    uint32_t set = 0;
    if (lane_on) {
        const uint64_t lrow = pixel / P.img_w;
        col = (int)(pixel - lrow * P.img_w);
        row = P.first_row + (int)lrow * P.row_stride;
        set = (uint32_t)P.rowperm[(size_t)row * P.num_sets + col] % P.num_sets;  // trace.rs:68-69
    }
    Stats st = {};
    double sr = 0.0, sg = 0.0, sb = 0.0;
    const uint32_t nchunks = (N + 63u) / 64u;
    for (uint32_t c = 0; c < nchunks; ++c) {
        const uint32_t i = i0 + c * 64u;
        if (lane_on && i < N) {
            Path p;
            p.sq = P.pix[(size_t)set * N + i];
            const double2 lens = P.disc[(size_t)set * N + i];
            p.r = primary_ray(P, row, col, p.sq, lens);
            path_begin(p);
            if (STATS) st.c[0]++;
            double Lr, Lg, Lb;
            while (shade_level<STATS, TRIS>(P, p, set, i, stk, stride, tstack, Lr, Lg, Lb, st)) {
            }
            fold_path(p, stk, stride, Lr, Lg, Lb);
            sr += Lr;  // trace.rs:82
            sg += Lg;
            sb += Lb;
        }
    }
    finish_pixel(P, lane_on, lane, seg_base, lpp, pixel, sr, sg, sb);
    flush_stats<STATS>(P, st, lane);
}

// ---------------------------------------------------------------------------
// REFILL variant (n*n >= 64): the wave keeps a cursor into its pixel's sample
// list; every iteration all live lanes advance one Scene::shade level, and the
// lanes whose path just ended are compacted (ballot + mbcnt prefix) onto the
// next unstarted samples.
// ---------------------------------------------------------------------------
template <bool STATS, bool TRIS>
__global__ __launch_bounds__(64 * FLUX_MAX_WAVES_PER_PIXEL, TRIS ? FLUX_WPE_WIDE : FLUX_WPE) void render_refill_kernel(const RenderParams P0) {
    const RenderParams &P = P0;  // (inside the pass loop: shadowed by the re-read view)
    extern __shared__ double lds_stack[];
#if FLUX_FAST
    __shared__ double part_store[FLUX_MAX_WAVES_PER_PIXEL * 3];  // per-wave totals of the pixel (K > 1): wave k's at [3 k + c]
    double *const part = part_store;
    constexpr uint32_t kPartStride = 3;
#else
    // STRICT: the per-wave totals go where the wave's own recursion stack was (level 0, the wave's lanes 0..2: dead once its
    // path loop has ended).  With a static array beside it, a block of four waves at max_trace_depth 5 took 40 960 + 96 B of LDS
    // and the CU held THREE such blocks (3 waves/SIMD); 40 960 B is exactly 32 of its 128 granules: four blocks, 4 waves/SIMD.
    // INVARIANTS this aliasing rests on (ADVICE round 5): (i) the recursion stack starts at lds_stack[0] and lane `tid`'s level-0 entry is
    // lds_stack[tid + c], c < 4 (stk = lds_stack + tid below; a level's stride is blockDim.x >= 64), so part[64 sub + c], c < 3, are level-0
    // words of wave `sub`'s OWN lanes 0..2 -- no other wave ever touches them; (ii) max_trace_depth >= 1, so level 0 exists (abi.hip
    // validates it); (iii) a wave writes its total after its path loop and before the block's barrier.  A layout change (the BVH stack
    // first, another stride) must move `part` with it: the static_assert below pins the one fact a compiler can check.
    double *const part = lds_stack;
    constexpr uint32_t kPartStride = 64;
    static_assert(kPartStride == 64, "per-wave totals alias level 0 of the wave's own lanes: one wave = 64 lanes");
#endif
    const int tid = threadIdx.x;
    const uint32_t lane = tid & 63;
    const int stride = blockDim.x;
    double *stk = lds_stack + tid;
    int *tstack = bvh_stack_base(lds_stack, P, stride) + tid;

    // One BLOCK = one pixel; its K = blockDim/64 waves take K contiguous slices of the pixel's sample list, so a
    // 16384-spp pixel is 4 work items of a quarter the length (the ragged end of a launch -- slots idling
    // while the last long pixels finish -- shrinks accordingly, which is what limits an 8-GPU frame).  K depends
    // on the sample count only (launch_plan.cpp), so the summation order, hence the image, does not depend on how
    // the frame is split over launches or GPUs.
    const uint32_t N = P.nsamp;
    const uint32_t K = blockDim.x >> 6, sub = (uint32_t)__builtin_amdgcn_readfirstlane(tid >> 6);  // a scalar: see render_split_kernel
    const uint32_t s_lo = (uint32_t)((uint64_t)N * sub / K), s_hi = (uint32_t)((uint64_t)N * (sub + 1) / K);
    const uint64_t wave = blockIdx.x;
    int lrow = 0, col = 0, row = 0;
    uint32_t set = 0;
    uint64_t pixel = 0;  // index of this block's pixel in the output buffer
    const bool wave_on = map_wave(P, wave, lrow, col, row, set, pixel);  // block-uniform
    // one wave = one pixel: tell the compiler these are uniform, so table bases live in SGPRs
    set = (uint32_t)__builtin_amdgcn_readfirstlane((int)set);
    col = __builtin_amdgcn_readfirstlane(col);
    row = __builtin_amdgcn_readfirstlane(row);

    Stats st = {};
    double sr = 0.0, sg = 0.0, sb = 0.0;
    if (wave_on) {
        const double2 *pix = P.pix + (size_t)set * N;
        const double2 *disc = P.disc + (size_t)set * N;

        uint32_t next = s_lo;  // wave-uniform cursor: first unstarted sample of this wave's slice
        uint32_t i = 0;
        bool live = false;
        bool want = true;  // lane needs a new sample
        Path p;
        path_begin(p);
        p.sq = make_double2(0.0, 0.0);
        p.r = Ray{0, 0, 0, 0, 0, 1};
        for (;;) {
            const RenderParams &P = relaunder_params(next);  // kernel arguments re-read per pass (see relaunder_params)
            // --- compaction: hand the next samples to the lanes that are free
            const unsigned long long freemask = ballot64(want);
            if (freemask) {
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(freemask >> 32),
                                                                __builtin_amdgcn_mbcnt_lo((uint32_t)freemask, 0u));
                if (want) {
                    i = next + rank;
                    live = i < s_hi;
                    if (live) {
                        p.sq = pix[i];
                        p.r = primary_ray(P, row, col, p.sq, disc[i]);
                        path_begin(p);
                        if (STATS) st.c[0]++;
                    }
                    want = false;
                }
                next += (uint32_t)__popcll(freemask);
                if (next > s_hi) next = s_hi;
            }
            if (!any64(live)) break;
            FLUX_TRIP(P, 10);
            // --- one Scene::shade level for every live lane
            if (live) {
                double Lr, Lg, Lb;
                if (!shade_level<STATS, TRIS>(P, p, set, i, stk, stride, tstack, Lr, Lg, Lb, st)) {
                    fold_path(p, stk, stride, Lr, Lg, Lb);
                    sr += Lr;
                    sg += Lg;
                    sb += Lb;
                    live = false;
                    want = next < s_hi;  // nothing left to start -> lane retires
                }
            }
        }
    }
    if (K == 1) {
        finish_pixel(P, wave_on, lane, 0u, 64u, pixel, sr, sg, sb);
    } else {
        // the wave's total (wave_sum3's fixed tree), then the K wave totals in wave order: a fixed summation tree
        double r, g, b;
        wave_sum3(sr, sg, sb, r, g, b);
        if (lane == 0) {
            part[kPartStride * sub + 0] = r;
            part[kPartStride * sub + 1] = g;
            part[kPartStride * sub + 2] = b;
        }
        __syncthreads();
        if (sub == 0) {
            double tr = 0.0, tg = 0.0, tb = 0.0;
            for (uint32_t k = 0; k < K; ++k) {
                tr += part[kPartStride * k + 0];
                tg += part[kPartStride * k + 1];
                tb += part[kPartStride * k + 2];
            }
            // a one-lane "segment" holding the block total: finish_pixel scales, clamps and stores it
            finish_pixel(P, wave_on, lane, 0u, 1u, pixel, tr, tg, tb);
        }
    }
    flush_stats<STATS>(P, st, lane);
}

#if FLUX_FAST
// ---------------------------------------------------------------------------
// SPLIT variant (FAST, analytic scenes, n*n >= 64, <= 64 spheres): primary and secondary segments run in separate
// passes of the same wave.
//
// In the refill kernel a lane whose path ended takes the pixel's next sample at once, so one loop iteration mixes
// the two kinds of segment a path tracer has: PRIMARY segments -- all 64 lanes of a wave sample the SAME pixel, so
// their rays are nearly parallel, hit the same one or two shapes and shade with the same material -- and SECONDARY
// segments, whose rays go anywhere.  The mix pays the general price for both: the 12-sphere candidate filter runs for
// rays whose candidates are known in advance, and the coherent primaries shade under the divergent mask of the rest.
// Here instead:
//   phase A  64 fresh samples at a time (all lanes), Scene::hit restricted to the PIXEL's candidate spheres -- a
//            wave-uniform mask computed once per wave from the bundle of rays through the pixel and the lens, so the
//            sphere records are scalar operands and control flow is uniform -- then Scene::shade's first level; paths
//            that continue are compacted (ballot + mbcnt) into a 64-entry queue in LDS (ray, throughput, pixel
//            sample, index: 92 B per path);
//   phase B  the refill loop on secondary segments only: free lanes pop queued paths; when the queue is empty and a
//            lane is free, phase A runs again.  Lanes are idle only while the wave's slice drains.
// Hit decisions are Scene::hit's (the pixel mask is a conservative superset, the exact tests and the tie rule are the
// same), so path statistics equal the CPU checker's exactly; the image equals the refill kernel's up to the order in which
// a pixel's samples are summed (still a fixed order: bit-reproducible, independent of how the frame is sharded).
// ---------------------------------------------------------------------------
// The two queues' layouts, kQueueBytesPerWave and kHitQBytesPerSlot, are in flux_plan.h: the launch plan reserves their LDS.
// A queued path: ox oy oz dx dy dz tr tg tb, the sample index and Path::self (GlossySpecular's re-mapped sample is read from the
// glossy-lobe table by the sample index, so the pixel sample itself is dead after the primary ray).
// The hit queue (plan_render chooses C per scene): C slots per wave, an array of structures (flux_plan.h): a slot is 17 dwords -- the
// seven doubles as dword pairs on even dwords, then the three ints --, so one multiply-add gives a lane its slot's address and every field is a
// constant offset from it (field-major arrays of C entries, C known only at the launch, cost an address addition per field), and the
// odd stride keeps a wave's accesses off each other's LDS banks.
// Phase B only CLASSIFIES its hits; a continuing hit is parked here -- the segment o d and its hit distance t (8 B each), the hit-record
// index and the depth (one int), the sample index (int) and the path's throughput -- and its bounce runs later, in a pass whose free
// lanes take a full batch of parked hits at once (bounce_parked_hit), instead of under the sparse mask of the scan's survivors.
// The throughput is kept as the list of the path's earlier bounce records, `bits` per bounce in one int (68 B a slot; three doubles,
// 88 B a slot, was measured slower: DESIGN.md §4, the hit queue): without long-form glossy weights (P.glossy_long) a bounce
// of an analytic shape multiplies the throughput by its record's (fr, fg, fb) and nothing else, so the product recomputed front to back from the block's LDS copy of the records is bit
// for bit the running one -- and so is the same product formed once per scene on the host: where the context holds the throughput
// product table (RenderParams::tput, flux_plan.h tput_index) the take gathers the list's product from it.  Every decision of the pass loop is a count (wave-uniform), so frames stay bit-reproducible.

// The spheres a primary ray of pixel (row, col) can hit: a conservative wave-uniform mask (bit = scan index).
// Every primary ray starts on the lens, |o - eye| <= R = lens_radius (to_poisson_disc maps into the unit disc,
// lib.rs:144-182), and passes through the point Fp = eye + x k U + y k V - f W of the focal plane (trace.rs:44-51:
// o + the un-normalised direction), x, y in the pixel's footprint (trace.rs:72-73).  With Fc the footprint's centre,
// h its half diagonal, a = Fc - eye: at parameter lam >= 0 the ray point (1-lam) o + lam Fp is within
// |1-lam| R + lam h <= R + lam (R + h) of the axis point eye + lam a.  A sphere (p, r) can only be hit if some axis
// point is within r + that radius; minimising over lam (unconstrained: a superset; for beta < 1) gives
//     d_perp sqrt(1 - beta^2) + beta (eye - p).a^  <=  r + R,   beta = (R + h) / |a|,
// d_perp the distance from p to the axis line.  `in_mask`: spheres that contain the whole lens (every primary ray
// starts strictly inside: their hit is the exit point, see the deferred-inside rule below).
// `in_t0`: for the FIRST sphere of in_mask (the environment, as a rule) a distance within which every point a primary ray of this pixel
// reaches is still inside that sphere by a margin: |point - centre| <= |eye - centre| + R + t, so t <= r (1 - 1e-6) - |eye - centre| - R
// will do.  scan_shapes_primary skips the sphere's test for a wave whose lanes all hold a nearer hit than that -- one compare per
// lane instead of the dozen operations of the exact margin test (which stays, behind it).  -1 when there is no such sphere.
__device__ __forceinline__ void pixel_sphere_mask(const RenderParams &P, int row, int col, uint32_t lane,
                                                  unsigned long long &cand_mask, unsigned long long &in_mask, double &in_t0) {
    const double xc = P.aps * (((double)col - P.half_w) + 0.5) * P.factor;
    const double yc = P.aps * (((double)(P.img_h - row) - P.half_h) + 0.5) * P.factor;
    const double ax = xc * P.Ux + yc * P.Vx - P.focal * P.Wx;
    const double ay = xc * P.Uy + yc * P.Vy - P.focal * P.Wy;
    const double az = xc * P.Uz + yc * P.Vz - P.focal * P.Wz;
    const double L2 = ax * ax + ay * ay + az * az;
    const double L = sqrt(L2);
    const double ulen = sqrt(P.Ux * P.Ux + P.Uy * P.Uy + P.Uz * P.Uz), vlen = sqrt(P.Vx * P.Vx + P.Vy * P.Vy + P.Vz * P.Vz);
    const double R = fabs(P.lens_radius) * (1.0 + 1e-9) * fmax(ulen, vlen);
    const double hx = 0.5 * fabs(P.aps * P.factor) * ulen, hy = 0.5 * fabs(P.aps * P.factor) * vlen;
    const double h = sqrt(hx * hx + hy * hy) * (1.0 + 1e-9);
    const double beta = (R + h) / L;
    bool cand = false, in = false;
    double t0 = -1.0;
    if ((int)lane < P.n_sph) {
        const DevScanSphere S = P.fsph[lane];
        const double ex = P.ex - S.px, ey = P.ey - S.py, ez = P.ez - S.pz;
        const double ee = ex * ex + ey * ey + ez * ez;
        const double ea = (ex * ax + ey * ay + ez * az) / L;  // (eye - p) . a^
        const double dperp = sqrt(fmax(ee - ea * ea, 0.0));
        const double rad = sqrt(S.rr);
        const double lhs = dperp * sqrt(fmax(1.0 - beta * beta, 0.0)) + beta * ea;
        const double slack = 1e-9 * (1.0 + rad + sqrt(ee));
        // negated comparisons: anything not provably clear (NaN, beta >= 1, L == 0) stays a candidate
        // (beta >= 1: the bundle's cone opens wider than 45 degrees and the bound above no longer holds -- keep everything)
        cand = !(lhs > rad + R + slack) || !(beta < 1.0);
        in = sqrt(ee) + R + slack < rad;
        t0 = rad * (1.0 - 1e-6) - (sqrt(ee) + R + slack);
    }
    cand_mask = ballot64(cand);
    in_mask = ballot64(in) & cand_mask;
    in_t0 = -1.0;
    if (in_mask) {  // (wave-uniform) the first such sphere's lane holds the bound
        const int k = __builtin_ctzll(in_mask);
        in_t0 = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(t0), k), __builtin_amdgcn_readlane(__double2loint(t0), k));
    }
}

// Phase B's ONE vote of a pass, in front of scan_shapes_fast's ZF instantiations: the lanes (of those that trace) that keep the wave out
// of ZF = 0.  As before: a lane with direction.z == 0, and a lane whose origin is beyond the filter's and the self-skip rule's range,
// |o|^2 >= 0.999e6 in f32 or NaN -- so in a wave that passes, every component of every origin is finite and below 1e3 (an infinite or
// NaN component, or one beyond f32, makes the sum infinite or NaN).  (|o|^2 and o.u in f32 exactly as filter_ray32_f forms them: the
// compiler merges the two.)
// AXIS (the instantiation for a first plane whose normal lies on that axis): the reduced plane test of ZF = 0 also needs, of every lane
// (flux_plane_axis.h plane_axis_admits, plane_axis_admits_b -- the CPU test holds this vote to that predicate),
//     plane_div_admits(d_a)    d_a not zero and of a size the reduced arm's unscaled division takes: one class test of (float)d_a,
//                              which the filter forms anyway;
//     d_x, d_y, d_z finite     |o.u| < 3e38 in f32, one compare of a value the filter forms anyway: an infinite or NaN component of d
//                              (or one beyond f32) times a finite o_i is infinite or -- o_i = 0 -- NaN, and the fused sum that takes it
//                              in stays infinite or NaN.  A NaN d_a fails here.
// Two more vector instructions a pass.
template <int AXIS>
__device__ __forceinline__ unsigned long long split_rare_lanes(const Ray &r) {
    const float ofx = (float)r.ox, ofy = (float)r.oy, ofz = (float)r.oz;
    const float oo32 = __builtin_fmaf(ofz, ofz, __builtin_fmaf(ofy, ofy, ofx * ofx));
    unsigned long long rare = ballot64(r.dz == 0.0) | ballot64(!(oo32 < 0.999e6f));
    if (AXIS != kPlaneAxisNone) {
        const float ou32 = __builtin_fmaf(ofz, (float)r.dz, __builtin_fmaf(ofy, (float)r.dy, ofx * (float)r.dx));
        rare |= ballot64(!(__builtin_fabsf(ou32) < 3.0e38f));
        rare |= ballot64(true) & ~plane_div_admits_lanes(AXIS == kPlaneAxisX ? r.dx : AXIS == kPlaneAxisY ? r.dy : r.dz);
    }
    return rare;
}

// Scene::hit for a primary ray against the pixel's candidates: planes and disks as in scan_shapes_fast, then the exact sphere
// test (shapes.rs:176-214 along the unit direction) with the sphere record in SGPRs and a wave-uniform trip count.
template <bool TYP, int AXIS = 0>
__device__ __forceinline__ void scan_shapes_primary(const RenderParams &P, const Ray &r, unsigned long long cand_mask,
                                                    unsigned long long in_mask, double in_t0, bool valid, unsigned long long valid_m,
                                                    int &best, double &tb) {
    (void)valid;
    (void)valid_m;  // the lane mask of `valid`
    int best_id = -1;
    const double tmin = P.t_min;  // (T_MIN from the kernel arguments, as in scan_shapes_fast)
    int j0 = 0;
    if (P.n_pln > 0) {  // the first plane: one compare and one select (scan_shapes_fast)
        const DevScanPlane &S = P.fpln[0];
        // AXIS (the instantiation for a plane whose stored normal lies on that axis): num = p_a - o_a, den = d_a, the general t bit for
        // bit (flux_plane_axis.h) in a wave whose valid lanes all hold a d_a of ordinary size (plane_div_admits: its f32 image a normal
        // number, which a zero, a NaN and an infinity are not) -- one conversion and ONE class test a pass.  The rest of
        // the predicate is the host's: it sets the axis only for a camera of finite scalars below 1e60 (plane_axis_camera_ok), the sample
        // tables hold points of the unit square and the unit disc, so primary_ray_px's origin is finite and of that size, and its
        // direction is a finite vector times ONE frsqrt -- finite in all three components or NaN in all three, and a NaN d_a has failed
        // the compare.  Any other wave forms the dot products in full.  (A zero num needs no guard: scan_shapes_fast.)
        bool reduced = false;
        if (AXIS != kPlaneAxisNone) {
            const double da = AXIS == kPlaneAxisX ? r.dx : AXIS == kPlaneAxisY ? r.dy : r.dz;
            reduced = (valid_m & ~plane_div_admits_lanes(da)) == 0ull;
        }
        double num, den, t;
        if (AXIS != kPlaneAxisNone && reduced) {
            plane_axis_num_den(AXIS, S.px, S.py, S.pz, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz, num, den);
            t = plane_div_unscaled(num, den);  // (the vote: no operand of this division is scaled, nothing is fixed up)
        } else {
            num = (S.px - r.ox) * S.nx + (S.py - r.oy) * S.ny + (S.pz - r.oz) * S.nz;
            den = r.dx * S.nx + r.dy * S.ny + r.dz * S.nz;
            t = num / den;
        }
        best = t > tmin ? P.n_sph : -1;
        best_id = S.id;
        tb = t;
        j0 = 1;
    }
    for (int j = j0; j < P.n_pln; ++j) {
        const DevScanPlane &S = P.fpln[j];
        const double num = (S.px - r.ox) * S.nx + (S.py - r.oy) * S.ny + (S.pz - r.oz) * S.nz;
        const double den = r.dx * S.nx + r.dy * S.ny + r.dz * S.nz;
        const double t = num / den;
        if (t > tmin && (best < 0 || t < tb)) {
            best = P.n_sph + j;
            best_id = S.id;
            tb = t;
        }
    }
    if (!TYP) {  // (TYP: a scene without disks or boxes, as in scan_shapes_fast)
        scan_disks(P, r, tmin, best, best_id, tb);
        scan_boxes(P, r, tmin, best, best_id, tb);
    }
    // a primary direction is normalize(...) (trace.rs:44-51): already the unit direction the quadratic is solved along
    const double rs = 1.0, ux = r.dx, uy = r.dy, uz = r.dz, len = 1.0;
    const bool zflat = r.dz == 0.0, any_zflat = any64(zflat);  // box_z_nan_miss, as in scan_shapes_fast
    for (int pass = 0; pass < 2; ++pass) {
        unsigned long long todo = pass == 0 ? (cand_mask & ~in_mask) : in_mask;
        // the first sphere that contains the lens: nothing to test while every lane's hit is nearer than pixel_sphere_mask's bound
        // (the hit lies inside the sphere by a margin, the sphere's exit point behind it)
        if (pass == 1 && todo && (valid_m & ~(ballot64(best >= 0) & ballot64(tb <= in_t0))) == 0ull) todo &= todo - 1;
        while (todo) {
            const int k = __builtin_ctzll(todo);  // wave-uniform
            todo &= todo - 1;
            const DevScanSphere S = P.fsph[k];
            FLUX_TRIP(P, 13);
            FLUX_CENSUS(P, 1);
            const double tx = r.ox - S.px, ty = r.oy - S.py, tz = r.oz - S.pz;
            const double hb = sphere_hb(tx, ty, tz, ux, uy, uz);
            const double c = __builtin_fma(tx, tx, __builtin_fma(ty, ty, __builtin_fma(tz, tz, -S.rr)));
            if (pass == 1) {
                // origin inside (the whole lens is): the hit is the exit point, farther than any interior point --
                // skipped when every lane's best hit already lies inside by a clear margin (scan_shapes_fast)
                const double tu = tb * len;
                const double g = __builtin_fma(tu, __builtin_fma(2.0, hb, tu), c);
                if ((valid_m & ~(ballot64(best >= 0) & ballot64(g < -1e-7 * S.rr))) == 0ull) continue;  // every lane skips
            }
            const double dq = __builtin_fma(hb, hb, -c);
            const double e = fastmath::fsqrt_nonneg(__builtin_fmax(dq, 0.0));
            double t = (-hb - e) * rs;             // shapes.rs:189
            if (!(t > tmin)) t = (-hb + e) * rs;  // shapes.rs:201
            bool ok = dq >= 0.0 && t > tmin;      // shapes.rs:181-183 (NaN fails both, as in the reference)
            if (any_zflat) {
                if (zflat && box_z_nan_miss(P, r, k)) ok = false;
            }
            if (ok) {
                bool take = best < 0 || t < tb;
                if (!take && t == tb) take = best >= P.n_sph ? P.frec[k].orig_id < best_id : k < best;
                if (take) {
                    best = k;
                    tb = t;
                }
            }
        }
    }
}

// A double of a hit-queue entry: entries are arrays of dwords at 4-byte alignment (flux_plan.h), read and written as dword pairs.
__device__ __forceinline__ double lds_dword_pair(const uint32_t *p) { return __hiloint2double((int)p[1], (int)p[0]); }
__device__ __forceinline__ void lds_dword_pair_store(uint32_t *p, double v) {
    p[0] = (uint32_t)__double2loint(v);
    p[1] = (uint32_t)__double2hiint(v);
}

// Entry k of a wave's pool (flux_plan.h hitq_entry_dword: slot C - 1 - k), its byte offset formed with a 24-bit multiply so that it
// and the pool's address are one v_mad_u32_u24 (C is a few hundred at the most).
__device__ __forceinline__ uint32_t *hitq_entry(uint32_t *pool, uint32_t C, uint32_t k) {
    return reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(pool) + __umul24(C - 1u - k, (uint32_t)kHitQBytesPerSlot));
}

// Phase A's shading step (both loops of the split kernel), entered by the lanes of `valid`.  A wave's 64 primaries sample one pixel, so
// mostly they all hit the same shape (demo2: 68 % of the pixels see nothing but the floor).  One vote -- every active lane holds the
// hit of the first active one, -1 for a miss included; the lanes past the slice's end are not active here, so their copy of the last
// sample has no say -- and the step runs with that hit as a scalar (shade_hit_fast's UNI).  A wave that fails the vote, and every wave
// of a launch with uni_a == 0 (FLUX_SPLIT_UNIFORM_A=0, launch_plan.cpp), runs the general step.  Same values either way.
// (census sections 16 / 17: the passes that take the uniform step / the general one)
template <bool STATS, bool TYP, bool UNIFORM_A, int LF>
__device__ __forceinline__ bool shade_primary_hits(const RenderParams &P, Path &p, uint32_t set, uint32_t ia, int hit, double t, double &Lr,
                                                   double &Lg, double &Lb, Stats &st, const char *frec_lds, int uni_a) {
    if (UNIFORM_A) {
        const int hu = __builtin_amdgcn_readfirstlane(hit);
        if (uni_a != 0 && ballot64(hit != hu) == 0ull) {
            FLUX_CENSUS(P, 16);
            return shade_hit_fast<STATS, false, true, TYP, true, true, false, true, LF>(P, p, set, ia, hu, -1, t, Lr, Lg, Lb, st, 3, frec_lds);
        }
    }
    FLUX_CENSUS(P, 17);
    return shade_hit_fast<STATS, false, true, TYP, true>(P, p, set, ia, hit, -1, t, Lr, Lg, Lb, st, 3, frec_lds);
}
// The instantiations of render_split_kernel whose phase A has the uniform step: those that hold it within the kernel's 96 registers
// without a spill (DESIGN.md section 4, profiles/r12_uniform_phase_a/registers.txt) -- every one with the hit queue, and TYP with the
// ray queue.  The other two ray-queue instantiations stand at 96 and 95 registers without it and would spill 28 and 22 more.
constexpr bool split_uniform_a(bool TYP, bool HQ) { return HQ || TYP; }
// ... and where that step takes a flat Matte record's lobe frame from the table (RenderParams::lobe_frame), and how (kLobeEarly /
// kLobeLate above): every such instantiation but <!MAX32, !TYP, HQ>, which spills twelve scalar registers as it stands and would spill
// four more with the arm (profiles/r13_lobe_frames/registers.txt): it keeps the parent's code.
constexpr int split_lobe_frames(bool MAX32, bool TYP, bool HQ) {
    return !split_uniform_a(TYP, HQ) ? kLobeOff : TYP ? kLobeEarly : MAX32 ? kLobeLate : kLobeOff;
}

// HQ: phase B parks its continuing hits in the hit queue of hq_cap slots (see kHitQBytesPerSlot); hq_th = H, hq_bits the
// bounce list's bits per entry.  Without HQ (scenes the queue does not fit, see launch_plan.cpp plan_render): the 64-entry ray queue and phase B's
// bounce at once, in the lanes that continue.
// AXIS: the axis of the first scan plane's stored normal (flux_plane_axis.h kPlaneAxisX/Y/Z), or 0.  TYP only: the launch takes the
// instantiation of RenderParams::plane_axis, and both scans take that plane's test in its reduced form (scan_shapes_primary,
// scan_shapes_fast).  A template argument and not a test of the field: with scalar branches on the field the frame was 3.6 % SLOWER than
// without the reduced form (146.6 against 141.5 ms), as a constant it is straight-line code (DESIGN.md section 4).
template <bool STATS, bool MAX32, bool TYP, bool HQ = false, int AXIS = 0>
__global__ __launch_bounds__(64 * FLUX_MAX_WAVES_PER_PIXEL, FLUX_WPE_SPLIT) void render_split_kernel(const RenderParams P0, int hq_cap, int hq_th,
                                                                                                  int hq_bits, int uni_a) {
    (void)hq_cap;
    (void)hq_th;
    (void)hq_bits;
    const RenderParams &P = P0;  // (inside the pass loop: shadowed by the re-read view)
    extern __shared__ double lds_stack[];
    __shared__ double part[FLUX_MAX_WAVES_PER_PIXEL][3];  // per-wave totals of the pixel (K > 1)
    const int tid = threadIdx.x;
    const uint32_t lane = tid & 63;
    const uint32_t N = P.nsamp;
    // the wave's index in the block as a SCALAR: the slice bounds, the sample cursor and the queue count derived from it are then wave-uniform
    // for the compiler too -- scalar registers and scalar arithmetic instead of three VGPRs and a dozen VALU instructions per pass
    const uint32_t K = blockDim.x >> 6, sub = (uint32_t)__builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t s_lo = (uint32_t)((uint64_t)N * sub / K), s_hi = (uint32_t)((uint64_t)N * (sub + 1) / K);
    // (the scene records FIRST, at an LDS address the compiler knows; the queues behind them)
    // (TYP: a scene without boxes, whose six records each the general count adds)
    const int n_rec = TYP ? P.n_sph + P.n_pln + P.n_dsk : hit_records(P);
    const size_t scene_lds_bytes = (size_t)n_rec * sizeof(DevHitRec) + (size_t)P.n_sph * sizeof(DevScanSphere);
    double *q = lds_stack + scene_lds_bytes / 8 + (size_t)sub * (HQ ? (size_t)hq_cap * kHitQBytesPerSlot / 8 : kQueueBytesPerWave / 8);
    int *qi = reinterpret_cast<int *>(q + (size_t)kQueueDoubles * 64);  // the ray queue: [field][slot]; the hit queue's pool starts at q
    // The scene's hit records (96 B per shape) and scan spheres (32 B) copied into the block's LDS behind the queues: the per-lane gathers
    // of the shading step and of the candidate loop -- dependent loads in the middle of a pass, ~600 cycles each from the L2 -- become
    // LDS reads (~100).  The launch plan reserves the bytes (plan_render: the split kernel serves scenes whose records fit 16 KiB).
    const char *const frec_lds = reinterpret_cast<const char *>(lds_stack);
    const char *const fsph_lds = frec_lds + (size_t)n_rec * sizeof(DevHitRec);
    {
        uint32_t *dst = reinterpret_cast<uint32_t *>(const_cast<char *>(frec_lds));
        const uint32_t nrec_w = (uint32_t)n_rec * (uint32_t)(sizeof(DevHitRec) / 4), nsph_w = (uint32_t)P.n_sph * 8u;
        const uint32_t *src_r = reinterpret_cast<const uint32_t *>(P.frec), *src_s = reinterpret_cast<const uint32_t *>(P.fsph);
        for (uint32_t w = (uint32_t)tid; w < nrec_w; w += blockDim.x) dst[w] = src_r[w];
        for (uint32_t w = (uint32_t)tid; w < nsph_w; w += blockDim.x) dst[nrec_w + w] = src_s[w];
        __syncthreads();
    }
    const uint64_t wave = blockIdx.x;
    int lrow = 0, col = 0, row = 0;
    uint32_t set = 0;
    uint64_t pixel = 0;
    const bool wave_on = map_wave(P, wave, lrow, col, row, set, pixel);  // block-uniform
    set = (uint32_t)__builtin_amdgcn_readfirstlane((int)set);
    col = __builtin_amdgcn_readfirstlane(col);
    row = __builtin_amdgcn_readfirstlane(row);

    Stats st = {};
    double sr = 0.0, sg = 0.0, sb = 0.0;
    if (HQ && wave_on) {
        unsigned long long cand_mask, in_mask;
        double in_t0;
        pixel_sphere_mask(P, row, col, lane, cand_mask, in_mask, in_t0);
        const uint32_t C = (uint32_t)hq_cap, H = (uint32_t)hq_th;
        const uint32_t bmask = (1u << hq_bits) - 1u;
        const DevHitRec *const recs = reinterpret_cast<const DevHitRec *>(frec_lds);
        uint32_t *const pool = reinterpret_cast<uint32_t *>(q);  // this wave's C entries (flux_plan.h hitq_entry_dword)
        uint32_t next = s_lo;  // wave-uniform cursor: first unstarted sample of this wave's slice
        uint32_t nhit = 0;     // wave-uniform: parked hits, entries 0 .. nhit-1 (entry k in slot C-1-k: the newest at C - nhit)
        constexpr int kDeadDepth = 0x7fffffff;  // (as in the loop below: "no path" kept in the depth)
        // Every lane is free at the top of a pass: the scan of the pass before ended or parked each of its paths.  So no path state is
        // carried from pass to pass -- only the sums, the statistics and the two counts.
        for (;;) {
            const RenderParams &P = relaunder_params(next + nhit);  // kernel arguments re-read per pass (see relaunder_params)
            uint32_t set_p = set;
            unsigned long long cand_p = cand_mask, in_p = in_mask;
            asm("" : "+s"(set_p) : "s"(next));
            asm("" : "+s"(cand_p), "+s"(in_p) : "s"(next));
            Path p;
            path_begin(p);
            p.depth = kDeadDepth;
            p.sq = make_double2(0.5, 0.5);
            uint32_t i = 0;
            uint32_t ml = 0;  // the records of the path's bounces so far, entry k at bit k * hq_bits
            // ---- phase A, while fewer than H hits are parked and the queue has room for all 64 continuations: samples next .. next+63,
            //      their continuing paths stay in their lanes
            const bool run_a = next < s_hi && nhit < H && hitq_admits_phase_a(C, nhit);
            if (run_a) {
                FLUX_TRIP(P, 12);
                FLUX_CENSUS(P, 0);
                // the batch's samples: slots next .. next+63 of the set's processing order (flux_sample_order.h: a permutation of 0 .. N-1,
                // so every sample is still traced once).  `valid`, the cursor and the primary ray's two tables (the set's copies in this order,
                // DevSetRows::pix_o / disc_o) go by the SLOT; the shading step's tables, the parked hit's sample word and the statistics by
                // the sample index ia read from it.  Lanes past the slice's end read the slice's
                // last slot (see the ray-queue loop below).
                const uint32_t slot_a = next + lane;
                const bool valid = slot_a < s_hi;
                const unsigned long long valid_m = ballot64(slot_a < s_hi);
                const uint32_t kc_a = slot_a < s_hi ? slot_a : s_hi - 1u;
                const uint32_t ia = gather_global<uint32_t>(set_rows_of(P, set_p).order, kc_a << 2);
                next = (s_hi - next) > 64u ? next + 64u : s_hi;
                bool cont = false;
                // (the two primary-ray tables in processing order: consecutive slots, consecutive 16-byte entries)
                const double2 *pix = set_rows_of(P, set_p).pix_o;
                const double2 *disc = set_rows_of(P, set_p).disc_o;
                const char *pxc_b = reinterpret_cast<const char *>(P.pxc);
                const PixelConsts PX = PixelConsts{*reinterpret_cast<const double *>(pxc_b + ((uint32_t)col << 3)),
                                                   *reinterpret_cast<const double *>(pxc_b + ((uint32_t)(P.img_w + row) << 3)), P.fwx, P.fwy, P.fwz};
                {
                    p.sq = gather_global_d2(pix, kc_a << 4);
                    p.r = primary_ray_px(P, PX, p.sq, gather_global_d2(disc, kc_a << 4));
                    if (STATS && valid) {
                        st.c[0]++;
                        st.c[1]++;
                    }
                }
                int hit = -1;
                double t = 0.0;
                scan_shapes_primary<TYP, AXIS>(P, p.r, cand_p, in_p, in_t0, valid, valid_m, hit, t);
                p.depth = 1;
                if (valid) {
                    double Lr, Lg, Lb;
                    FLUX_CENSUS(P, 2);
                    cont = shade_primary_hits<STATS, TYP, split_uniform_a(TYP, HQ), split_lobe_frames(MAX32, TYP, HQ)>(P, p, set_p, ia, hit, t, Lr, Lg, Lb, st, frec_lds, uni_a);
                    if (cont && p.depth > P.max_depth) {  // scene.rs:164-165 on entry to the next level
                        cont = false;
                        Lr = Lg = Lb = 0.0;
                        if (STATS) st.c[7]++;
                    }
                    if (!cont) {
                        fold_path(p, nullptr, 0, Lr, Lg, Lb);
                        sr += Lr;  // trace.rs:82
                        sg += Lg;
                        sb += Lb;
                    }
                }
                i = ia;
                ml = (uint32_t)hit;
                if (!cont) p.depth = kDeadDepth;
            }
            // ---- free lanes take parked hits, newest first, and bounce them: when phase A did not run (H of them are parked, the
            //      queue is full, or the slice is used up), or when H of them fill free lanes phase A left, or when phase A cannot run
            //      again
            if (nhit) {
                const unsigned long long freemask = ballot64(p.depth == kDeadDepth);
                const uint32_t nfree = (uint32_t)__popcll(freemask);
                const uint32_t take = nfree < nhit ? nfree : nhit;
                if (!run_a || take >= H || !(next < s_hi && hitq_admits_phase_a(C, nhit))) {
                    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(freemask >> 32),
                                                                    __builtin_amdgcn_mbcnt_lo((uint32_t)freemask, 0u));
                    if (p.depth == kDeadDepth && rank < take) {
                        FLUX_CENSUS(P, 15);
                        const uint32_t *e = hitq_entry(pool, C, nhit - 1u - rank);
                        p.r.ox = lds_dword_pair(e + kHitQOx);
                        p.r.oy = lds_dword_pair(e + kHitQOy);
                        p.r.oz = lds_dword_pair(e + kHitQOz);
                        p.r.dx = lds_dword_pair(e + kHitQDx);
                        p.r.dy = lds_dword_pair(e + kHitQDy);
                        p.r.dz = lds_dword_pair(e + kHitQDz);
                        const double t = lds_dword_pair(e + kHitQT);
                        const int hd = (int)e[kHitQHitDepth];
                        i = e[kHitQSample];
                        const int hit = hd & 0xffff;
                        p.depth = hd >> 16;
                        ml = e[kHitQList];
                        // the list's bits: depth - 1 entries.  ml's bits above them are zero -- it was set to the first hit and has had
                        // one hit (< 2^hq_bits) or-ed in just above the list per bounce, below -- which tput_index relies on
                        const uint32_t list_bits = __umul24((uint32_t)(p.depth - 1), (uint32_t)hq_bits);
                        // the throughput, front to back as fast_bounce formed it (the first bounce's weight, then one product per bounce):
                        // read from the scene's product table where the context holds one (wave-uniform; flux_plan.h tput_index), ...
                        if (P.tput != nullptr) {
                            const uint32_t off = __umul24(tput_index(list_bits, ml), (uint32_t)kTputEntryBytes);
                            p.tr = gather_global<double>(P.tput, off);
                            p.tg = gather_global<double>(P.tput, off + 8u);
                            p.tb = gather_global<double>(P.tput, off + 16u);
                        } else {  // ... or multiplied up from the records
                            const DevHitRec &R0 = recs[ml & bmask];
                            p.tr = R0.fr;
                            p.tg = R0.fg;
                            p.tb = R0.fb;
#pragma unroll 1
                            for (int k = 1; k < p.depth - 1; ++k) {
                                const DevHitRec &Rk = recs[(ml >> (k * hq_bits)) & bmask];
                                p.tr *= Rk.fr;
                                p.tg *= Rk.fg;
                                p.tb *= Rk.fb;
                            }
                        }
                        ml |= (uint32_t)hit << list_bits;
                        bounce_parked_hit<STATS, TYP>(P, p, set_p, i, hit, t, st, 6, frec_lds);
                    }
                    nhit -= take;
                }
            }
            // the way out: nothing parked, the slice used up and no lane live (the scalar test first, as below)
            if (__builtin_expect((nhit | (s_hi - next)) == 0u, 0)) {
                if (!any64(p.depth != kDeadDepth)) break;
            }
            // ---- phase B: Scene::hit and the first half of Scene::shade (scene.rs:162-172) for every live lane; a path that ends is
            //      added to the lane's sums, a path that continues is parked
            FLUX_TRIP(P, 10);
            const bool live = p.depth != kDeadDepth;
            const SplitDepths depths = split_depths<split_depth_pair(TYP)>(P);  // (the limit and the cut's depth: one load, here)
            const bool trace = p.depth <= split_max_depth<split_depth_pair(TYP)>(P, depths);  // (live, and) scene.rs:164-165: a path beyond the depth limit ends with L = 0
            double Lr = 0.0, Lg = 0.0, Lb = 0.0;
            bool cont = false;
            int hit = -1;
            double t = 0.0;
            if (trace) {
                FLUX_CENSUS(P, 3);
                if (STATS) st.c[1]++;
                int facing;
                if (__builtin_expect(split_rare_lanes<AXIS>(p.r) != 0ull, 0))
                    scan_shapes_fast<true, true, MAX32, TYP, 1, true, AXIS>(P, p.r, p.self, hit, t, nullptr, fsph_lds, &facing);
                else
                    scan_shapes_fast<true, true, MAX32, TYP, 0, true, AXIS>(P, p.r, p.self, hit, t, nullptr, fsph_lds, &facing);
                cont = shade_hit_fast<STATS, false, true, TYP, false, false, true>(P, p, set_p, i, hit, -1, t, Lr, Lg, Lb, st, 0, frec_lds, facing);
                // The depth cut (launch_plan.cpp split_cut_depth): the child of a bounce at the depth limit ends with L = 0 untraced, so
                // the path ends here with the zeros above -- nothing parked, no take, no bounce, no pass spent on finding it dead.
                if (cont && p.depth == split_cut_depth<split_depth_pair(TYP)>(P, depths)) {
                    cont = false;
                    if (STATS) {  // what the skipped bounce and the skipped pass counted
                        const int kind = recs[hit].mat_kind;
                        if (kind == kMatMatte) st.c[2]++;
                        if (kind == kMatGlossy) st.c[3]++;
                        if (kind == kMatReflective) st.c[4]++;
                        st.c[7]++;
                    }
                }
            }
            if (live && !cont) {
                if (STATS && !trace) st.c[7]++;
                fold_path(p, nullptr, 0, Lr, Lg, Lb);
                sr += Lr;
                sg += Lg;
                sb += Lb;
            }
            const unsigned long long pmask = ballot64(cont);
            if (cont) {
                // (room: the queue held at most C - 64 hits when this pass's phase A ran, and a pass without it parks no more paths
                // than it took from the queue)
                uint32_t *e = hitq_entry(pool, C, nhit + __builtin_amdgcn_mbcnt_hi((uint32_t)(pmask >> 32),
                                                                                   __builtin_amdgcn_mbcnt_lo((uint32_t)pmask, 0u)));
                lds_dword_pair_store(e + kHitQOx, p.r.ox);
                lds_dword_pair_store(e + kHitQOy, p.r.oy);
                lds_dword_pair_store(e + kHitQOz, p.r.oz);
                lds_dword_pair_store(e + kHitQDx, p.r.dx);
                lds_dword_pair_store(e + kHitQDy, p.r.dy);
                lds_dword_pair_store(e + kHitQDz, p.r.dz);
                lds_dword_pair_store(e + kHitQT, t);
                e[kHitQHitDepth] = (uint32_t)(hit | (p.depth << 16));
                e[kHitQSample] = i;
                e[kHitQList] = ml;
            }
            nhit += (uint32_t)__popcll(pmask);
        }
    }
    if (!HQ && wave_on) {
        unsigned long long cand_mask, in_mask;
        double in_t0;
        pixel_sphere_mask(P, row, col, lane, cand_mask, in_mask, in_t0);

#ifdef FLUX_DEBUG_CLOCK
        long long lap_store[8] = {0, 0, 0, 0, 0, 0, 0, (long long)__builtin_readcyclecounter()};
        long long *lap = lap_store;
#else
        long long *lap = nullptr;
#endif
        uint32_t next = s_lo;   // wave-uniform cursor: first unstarted sample of this wave's slice
        uint32_t qcount = 0;    // wave-uniform: queued paths
        uint32_t i = 0;
        // Whether a lane holds a path is kept IN the path's depth: kDeadDepth = no path.  The loop votes on it four times a pass, and a
        // ballot of a compare is the compare's own result, where a ballot of a loop-carried boolean costs a 0/1 select and a second
        // compare (two VALU instructions each time).  kDeadDepth is above every depth limit, so `depth <= max_depth` covers "live" too.
        constexpr int kDeadDepth = 0x7fffffff;
        Path p;
        path_begin(p);
        p.depth = kDeadDepth;
        p.sq = make_double2(0.0, 0.0);
        p.r = Ray{0, 0, 0, 0, 0, 1};
        for (;;) {
            const RenderParams &P = relaunder_params(next + qcount);  // kernel arguments re-read per pass (see relaunder_params)
            // The pixel's sample set and its two sphere masks are re-defined per pass as far as the optimiser can see: what it derives
            // from them (set << 5 as a 64-bit pair for the table addresses, the masks' xor, two `!= 0` flags as 64-bit lane masks) is then
            // one scalar instruction at the use instead of a scalar register pair held across the loop -- the allocator had spilled
            // those pairs to VGPR lanes and fetched them back with v_readlane_b32 (a VALU instruction) in every pass.
            uint32_t set_p = set;
            unsigned long long cand_p = cand_mask, in_p = in_mask;
            asm("" : "+s"(set_p) : "s"(next));
            asm("" : "+s"(cand_p), "+s"(in_p) : "s"(next));
            // --- free lanes take queued paths (newest first); if lanes are still free the queue is empty: phase A makes
            //     the next 64 primaries' continuations and the free lanes take theirs at once, so every lane has a
            //     secondary segment to trace in each phase-B pass until the slice runs out
            auto pop = [&]() {
                const unsigned long long freemask = ballot64(p.depth == kDeadDepth);
                if (!freemask || !qcount) return;
                const uint32_t nfree = (uint32_t)__popcll(freemask);
                const uint32_t take = nfree < qcount ? nfree : qcount;
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(freemask >> 32),
                                                                __builtin_amdgcn_mbcnt_lo((uint32_t)freemask, 0u));
                if (p.depth == kDeadDepth && rank < take) {
                    const uint32_t slot = qcount - 1u - rank;
                    p.r.ox = q[0 * 64 + slot];
                    p.r.oy = q[1 * 64 + slot];
                    p.r.oz = q[2 * 64 + slot];
                    p.r.dx = q[3 * 64 + slot];
                    p.r.dy = q[4 * 64 + slot];
                    p.r.dz = q[5 * 64 + slot];
                    p.tr = q[6 * 64 + slot];
                    p.tg = q[7 * 64 + slot];
                    p.tb = q[8 * 64 + slot];
                    i = (uint32_t)qi[slot];
                    p.self = qi[64 + slot];
                    p.depth = 2;
                    p.nb = 1;
                }
                qcount -= take;
            };
            pop();
            lap_stamp(lap, 0);
            if (next < s_hi && any64(p.depth == kDeadDepth)) {  // a lane is still free => the queue is empty
                // ---- phase A: primary segments of samples next .. next+63
                FLUX_TRIP(P, 12);
                FLUX_CENSUS(P, 0);
                // (the batch's samples by the set's processing order, as in the hit-queue loop above: the slot decides `valid` and the
                // cursor, the sample index ia everything downstream)
                const uint32_t slot_a = next + lane;
                const bool valid = slot_a < s_hi;
                const unsigned long long valid_m = ballot64(slot_a < s_hi);
                // Lanes past the slice's end (the last pass of a slice only) take the slice's last slot: every lane has a ray, there is no
                // masked region and no default ray -- seven 64-bit moves a pass -- to define for the others; what such a lane computes is
                // never used (`valid` gates the shading step, `valid_m` the votes).
                const uint32_t kc_a = slot_a < s_hi ? slot_a : s_hi - 1u;
                const uint32_t ia = gather_global<uint32_t>(set_rows_of(P, set_p).order, kc_a << 2);
                next = (s_hi - next) > 64u ? next + 64u : s_hi;
                bool cont = false;
                Path pa;
                path_begin(pa);
                pa.sq = make_double2(0.5, 0.5);
                pa.r = Ray{0, 0, 0, 0, 0, 1};
                // (the pixel's rows of the two sample tables: addresses formed here, not held across the loop)
                // (the two primary-ray tables in processing order: consecutive slots, consecutive 16-byte entries)
                const double2 *pix = set_rows_of(P, set_p).pix_o;
                const double2 *disc = set_rows_of(P, set_p).disc_o;
                // primary_ray's per-pixel and per-frame constants, read where they are used (scalar loads from the context's tables and the
                // kernel arguments): held in scalar registers across the pass loop they were 10 of the 29 registers the allocator spilled
                // to VGPR lanes, and came back through v_readlane_b32 in every ray-generation step
                // (32-bit byte offsets, as set_rows_of)
                const char *pxc_b = reinterpret_cast<const char *>(P.pxc);
                const PixelConsts PX = PixelConsts{*reinterpret_cast<const double *>(pxc_b + ((uint32_t)col << 3)),
                                                   *reinterpret_cast<const double *>(pxc_b + ((uint32_t)(P.img_w + row) << 3)), P.fwx, P.fwy, P.fwz};
                {
                    pa.sq = gather_global_d2(pix, kc_a << 4);
                    pa.r = primary_ray_px(P, PX, pa.sq, gather_global_d2(disc, kc_a << 4));
                    if (STATS && valid) {
                        st.c[0]++;
                        st.c[1]++;
                    }
                }
                int hit = -1;
                double t = 0.0;
                scan_shapes_primary<TYP, AXIS>(P, pa.r, cand_p, in_p, in_t0, valid, valid_m, hit, t);
                if (valid) {
                    double Lr, Lg, Lb;
                    FLUX_CENSUS(P, 2);
                    cont = shade_primary_hits<STATS, TYP, split_uniform_a(TYP, HQ), split_lobe_frames(MAX32, TYP, HQ)>(P, pa, set_p, ia, hit, t, Lr, Lg, Lb, st, frec_lds, uni_a);
                    if (cont && pa.depth > P.max_depth) {  // scene.rs:164-165 on entry to the next level
                        cont = false;
                        Lr = Lg = Lb = 0.0;
                        if (STATS) st.c[7]++;
                    }
                    if (!cont) {
                        fold_path(pa, nullptr, 0, Lr, Lg, Lb);
                        sr += Lr;  // trace.rs:82
                        sg += Lg;
                        sb += Lb;
                    }
                }
                const unsigned long long qmask = ballot64(cont);
                if (cont) {
                    const uint32_t slot = __builtin_amdgcn_mbcnt_hi((uint32_t)(qmask >> 32),
                                                                    __builtin_amdgcn_mbcnt_lo((uint32_t)qmask, 0u));
                    q[0 * 64 + slot] = pa.r.ox;
                    q[1 * 64 + slot] = pa.r.oy;
                    q[2 * 64 + slot] = pa.r.oz;
                    q[3 * 64 + slot] = pa.r.dx;
                    q[4 * 64 + slot] = pa.r.dy;
                    q[5 * 64 + slot] = pa.r.dz;
                    q[6 * 64 + slot] = pa.tr;
                    q[7 * 64 + slot] = pa.tg;
                    q[8 * 64 + slot] = pa.tb;
                    qi[slot] = (int)ia;
                    qi[64 + slot] = pa.self;
                }
                qcount = (uint32_t)__popcll(qmask);
                lap_stamp(lap, 1);
                pop();
                lap_stamp(lap, 0);
            }
            // the way out: nothing queued, the slice used up (next <= s_hi always: one scalar test for both) and no lane live.  The scalar
            // test FIRST: it fails in every pass but a wave's last few, and the vote on `live` -- a loop-carried boolean: a 0/1 select and a
            // compare -- is then not taken
            if (__builtin_expect((qcount | (s_hi - next)) == 0u, 0)) {
                if (!any64(p.depth != kDeadDepth)) break;
            }
            // ---- phase B: one Scene::shade level (scene.rs:162-172: a secondary segment) for every live lane
            // (two-phase shading: no `continue` above -- with no lane live the `if`s below are simply not taken --, so the loop
            // has ONE back edge and the path state one definition per pass)
            FLUX_TRIP(P, 10);
            // a sequence of plain `if`s, none with an else, each changing its own part of the loop-carried state (see shade_hit_fast)
            const bool live = p.depth != kDeadDepth;
            const SplitDepths depths = split_depths<split_depth_pair(TYP)>(P);  // (the limit and the cut's depth: one load, here)
            const bool trace = p.depth <= split_max_depth<split_depth_pair(TYP)>(P, depths);  // (live, and) scene.rs:164-165: a path beyond the depth limit ends with L = 0
            // (Lr = Lg = Lb = 0 are six 64-bit moves a pass as the compiler lowers them -- once per nesting level.  Leaving the three
            // undefined and writing the zeros behind a vote on `depth > max_depth` removes the moves and was measured 1.0 % SLOWER, twice:
            // profiles/r06_experiments/ab_m20_m22_m23_r06z.log, ab_m29_m30_r06ag.log.)
            double Lr = 0.0, Lg = 0.0, Lb = 0.0;
            bool cont = false;
            if (trace) {
                FLUX_CENSUS(P, 3);
                if (STATS) st.c[1]++;
                int hit = -1;
                double t = 0.0;
                if (__builtin_expect(split_rare_lanes<AXIS>(p.r) != 0ull, 0))
                    scan_shapes_fast<true, true, MAX32, TYP, 1, false, AXIS>(P, p.r, p.self, hit, t, lap, fsph_lds);
                else
                    scan_shapes_fast<true, true, MAX32, TYP, 0, false, AXIS>(P, p.r, p.self, hit, t, lap, fsph_lds);
                cont = shade_hit_fast<STATS, false, true, TYP>(P, p, set_p, i, hit, -1, t, Lr, Lg, Lb, st, 0, frec_lds);
                // The depth cut (launch_plan.cpp split_cut_depth), as phase A's: a child beyond the depth limit ends here with the zeros
                // above, folded below with the throughput its bounce left -- the lane is free a pass earlier.
                if (cont && p.depth > split_cut_depth<split_depth_pair(TYP)>(P, depths)) {
                    cont = false;
                    if (STATS) st.c[7]++;
                }
            }
            if (live && !cont) {
                if (STATS && !trace) st.c[7]++;
                fold_path(p, nullptr, 0, Lr, Lg, Lb);
                sr += Lr;
                sg += Lg;
                sb += Lb;
                p.depth = kDeadDepth;
            }
            lap_stamp(lap, 5);
        }
#ifdef FLUX_DEBUG_CLOCK
        if (P.stats && lane == 0)
            for (int k = 0; k < 6; ++k) atomicAdd(P.stats + 10 + k, (unsigned long long)lap[k]);
#endif
    }
    const RenderParams &PE = P;
    if (K == 1) {
        finish_pixel(PE, wave_on, lane, 0u, 64u, pixel, sr, sg, sb);
    } else {
        // the wave's total (wave_sum3's fixed tree), then the K wave totals in wave order: a fixed summation tree
        double r, g, b;
        wave_sum3(sr, sg, sb, r, g, b);
        if (lane == 0) {
            part[sub][0] = r;
            part[sub][1] = g;
            part[sub][2] = b;
        }
        __syncthreads();
        if (sub == 0) {
            double tr = 0.0, tg = 0.0, tb = 0.0;
            for (uint32_t k = 0; k < K; ++k) {
                tr += part[k][0];
                tg += part[k][1];
                tb += part[k][2];
            }
            finish_pixel(PE, wave_on, lane, 0u, 1u, pixel, tr, tg, tb);
        }
    }
    flush_stats<STATS>(PE, st, lane);
}

// ---------------------------------------------------------------------------
// BVH variant (FAST, triangle scenes, n*n >= 64): persistent lanes with a traversal state machine.
// The refill kernel above runs one whole Scene::hit per lane per iteration; with a BVH that is a
// per-lane loop of 5..80 node visits with triangle tests inlined, and the wave waits for its slowest lane
// with the triangle code executed whenever ANY lane sits at a leaf (measured on the 1 M-triangle scene:
// 11 % of lanes active per VALU instruction).  Here instead:
//   * every lane keeps its traversal state (current node, LDS stack, best hit) across loop iterations;
//   * "while-while" traversal with postponed leaves: all traversing lanes descend until each holds a
//     leaf reference (or is done), then all test their leaf's triangles together;
//   * lanes whose traversal finished wait in state SHADE until FLUX_BVH_REFILL_AT of them have
//     gathered (or nobody is traversing any more); only then the wave runs the shading / refill / analytic
//     scan code for them and they re-enter traversal with their next ray (bounce or next sample), while the
//     other lanes simply keep their traversal state;
//   * the slab test runs in f32 (half the issue cost) against the builder's f32 boxes and is
//     conservative: with eps = 2^-24, inv = 1/d and o rounded to f32 and one rounding per fma perturb each
//     slab distance by < 3 eps (B + |o|) |inv| (B = largest |vertex coordinate|; a point inside a box has
//     |o + t d| <= B), so the slabs are widened by delta = 16 eps (B + |o|_inf):
//        t_lo = fma(lo, inv, -(o + delta) inv),   t_hi = fma(hi, inv, -(o - delta) inv)
//     (the same two formulas for either sign of inv); the exact f64 Moeller-Trumbore test decides.
// Hit selection is the brute-force rule (nearest t, lowest hit-order index on ties), so the image equals
// the refill kernel's up to the order in which a pixel's samples are summed.
// ---------------------------------------------------------------------------
constexpr int kTravDone = (int)0x80000000;
constexpr double kTravPad = 16.0 / 16777216.0;  // 16 * 2^-24

struct TravRay {
    float ix, iy, iz;     // 1 / d
    float lox, loy, loz;  // -(o + delta) / d
    float hix, hiy, hiz;  // -(o - delta) / d
};
// the same for boxes given on the 16-bit grid (flux_bvh.h DevNodeQ): coordinate = qmin + q step, so
//   t_lo = fma(lo, 1/d, -(o+delta)/d) = q (step/d) + (qmin/d - (o+delta)/d)   -- one fma per slab plane, as before
struct TravRayQ {
    float sx, sy, sz;     // step / d
    float lox, loy, loz;
    float hix, hiy, hiz;
};
__device__ __forceinline__ void trav_setup_q(const RenderParams &P, const TravRay &T, TravRayQ &Q) {
    Q.sx = P.bvh_qstep[0] * T.ix;
    Q.sy = P.bvh_qstep[1] * T.iy;
    Q.sz = P.bvh_qstep[2] * T.iz;
    Q.lox = __builtin_fmaf(P.bvh_qmin[0], T.ix, T.lox);
    Q.loy = __builtin_fmaf(P.bvh_qmin[1], T.iy, T.loy);
    Q.loz = __builtin_fmaf(P.bvh_qmin[2], T.iz, T.loz);
    Q.hix = __builtin_fmaf(P.bvh_qmin[0], T.ix, T.hix);
    Q.hiy = __builtin_fmaf(P.bvh_qmin[1], T.iy, T.hiy);
    Q.hiz = __builtin_fmaf(P.bvh_qmin[2], T.iz, T.hiz);
}
// slab test of a quantised box: same conservative test as box_hit32 (the box CONTAINS the f32 box by a full quantum,
// far more than the extra f32 roundings of step/d and qmin/d)
__device__ __forceinline__ bool box_hit_q(float lx, float ly, float lz, float hx, float hy, float hz, const TravRayQ &Q,
                                          float tb32, float &tnear) {
    const float x0 = __builtin_fmaf(lx, Q.sx, Q.lox), x1 = __builtin_fmaf(hx, Q.sx, Q.hix);
    const float y0 = __builtin_fmaf(ly, Q.sy, Q.loy), y1 = __builtin_fmaf(hy, Q.sy, Q.hiy);
    const float z0 = __builtin_fmaf(lz, Q.sz, Q.loz), z1 = __builtin_fmaf(hz, Q.sz, Q.hiz);
    const float tn = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fminf(z0, z1));
    const float tf = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1));
    tnear = tn;
    return tn <= tf && tf >= 0.0f && tn <= tb32;
}

__device__ __forceinline__ void trav_setup(const RenderParams &P, const Ray &r, TravRay &T) {
    const double tiny = 1e-20;  // |d| below this is treated as this: keeps every f32 product finite
    // 1 / d in f32 from the hardware's v_rcp_f32 (1 ulp) instead of three IEEE f64 divisions (13 instructions + a 16-cycle seed each):
    // the slab test runs in f32 anyway, and the SAME rounded 1 / d scales both terms of a slab distance, so its error is one more
    // relative 2^-24 on t -- the padding below (16 of them) covers 3 already spent and this one
    const float fx = (float)(fabs(r.dx) < tiny ? copysign(tiny, r.dx) : r.dx), fy = (float)(fabs(r.dy) < tiny ? copysign(tiny, r.dy) : r.dy),
                fz = (float)(fabs(r.dz) < tiny ? copysign(tiny, r.dz) : r.dz);
    T.ix = __builtin_amdgcn_rcpf(fx);
    T.iy = __builtin_amdgcn_rcpf(fy);
    T.iz = __builtin_amdgcn_rcpf(fz);
    const double ix = (double)T.ix, iy = (double)T.iy, iz = (double)T.iz;
    const double delta = kTravPad * (P.bvh_mag + fmax(fmax(fabs(r.ox), fabs(r.oy)), fabs(r.oz)));
    T.lox = (float)(-(r.ox + delta) * ix);
    T.loy = (float)(-(r.oy + delta) * iy);
    T.loz = (float)(-(r.oz + delta) * iz);
    T.hix = (float)(-(r.ox - delta) * ix);
    T.hiy = (float)(-(r.oy - delta) * iy);
    T.hiz = (float)(-(r.oz - delta) * iz);
}

__device__ __forceinline__ bool box_hit32(const float *lo, const float *hi, const TravRay &T, float tb32,
                                          float &tnear) {
    const float x0 = __builtin_fmaf(lo[0], T.ix, T.lox), x1 = __builtin_fmaf(hi[0], T.ix, T.hix);
    const float y0 = __builtin_fmaf(lo[1], T.iy, T.loy), y1 = __builtin_fmaf(hi[1], T.iy, T.hiy);
    const float z0 = __builtin_fmaf(lo[2], T.iz, T.loz), z1 = __builtin_fmaf(hi[2], T.iz, T.hiz);
    const float tn = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fminf(z0, z1));
    const float tf = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1));
    tnear = tn;
    return tn <= tf && tf >= 0.0f && tn <= tb32;
}

// float >= t (round to nearest, then one relative step up)
__device__ __forceinline__ float upper32(double t) { return (float)t * 1.0000005f; }

template <bool STATS>
__global__ __launch_bounds__(FLUX_BLOCK_THREADS, FLUX_WPE_BVH) void render_bvh_kernel(const RenderParams P0) {
    const RenderParams &P = P0;  // (inside the pass loop: shadowed by the re-read view)
    extern __shared__ double lds_stack[];
    const int tid = threadIdx.x;  // one wave per block (launch_plan.cpp)
    const uint32_t lane = tid & 63;
    // traversal stack [entry][lane] in LDS, addressed by BYTE offset (`sp` counts bytes: +-256 per entry, no multiply)
    char *tstack = reinterpret_cast<char *>(lds_stack) + tid * 4;
    constexpr int kEntry = 64 * 4;

    const uint32_t N = P.nsamp;
    const uint64_t wave = blockIdx.x;
    int lrow = 0, col = 0, row = 0;
    uint32_t set = 0;
    uint64_t pixel = 0;  // index of this wave's pixel in the output buffer
    const bool wave_on = map_wave(P, wave, lrow, col, row, set, pixel);  // wave-uniform
    // one wave = one pixel: tell the compiler these are uniform, so table bases live in SGPRs
    set = (uint32_t)__builtin_amdgcn_readfirstlane((int)set);
    col = __builtin_amdgcn_readfirstlane(col);
    row = __builtin_amdgcn_readfirstlane(row);

    Stats st = {};
    double sr = 0.0, sg = 0.0, sb = 0.0;
    if (wave_on) {
        const double2 *pix = P.pix + (size_t)set * N;
        const double2 *disc = P.disc + (size_t)set * N;

        enum { kIdle = 0, kWant = 1, kFresh = 2, kTrav = 3, kShade = 4 };
        int mode = kWant;
        uint32_t next = 0;  // wave-uniform cursor: first unstarted sample
        uint32_t i = 0;
        Path p;
        path_begin(p);
        p.sq = make_double2(0.0, 0.0);
        p.r = Ray{0, 0, 0, 0, 0, 1};
        TravRay T = {};
        TravRayQ TQ = {};
        int cur = kTravDone, sp = 0;
        int hit_rec = -1, best = -1, bslot = -1;
        double tb = 0.0;
        float tb32 = 3.0e38f;
        for (;;) {
            const RenderParams &P = relaunder_params(next);  // kernel arguments re-read per pass (see relaunder_params)
            // --- (1) Scene::shade after the hit, for the lanes whose traversal is complete
            if (mode == kShade) {
                FLUX_TRIP_LANES(P, 10);
                double Lr, Lg, Lb;
                bool cont = shade_hit<STATS, true>(P, p, set, i, bslot >= 0 ? best : hit_rec, bslot, tb, nullptr, 0,
                                                   Lr, Lg, Lb, st);
                if (cont && p.depth > P.max_depth) {  // scene.rs:164-165 on entry to the next level
                    cont = false;
                    Lr = Lg = Lb = 0.0;
                    if (STATS) st.c[7]++;
                }
                if (cont) {
                    mode = kFresh;
                } else {
                    fold_path(p, nullptr, 0, Lr, Lg, Lb);
                    sr += Lr;  // trace.rs:82
                    sg += Lg;
                    sb += Lb;
                    mode = kWant;
                }
            }
            // --- (2) compaction: hand the pixel's next samples to the free lanes (ballot + mbcnt prefix)
            const unsigned long long freemask = ballot64(mode == kWant);
            if (freemask) {
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(freemask >> 32),
                                                                __builtin_amdgcn_mbcnt_lo((uint32_t)freemask, 0u));
                if (mode == kWant) {
                    i = next + rank;
                    if (i < N) {
                        p.sq = pix[i];
                        p.r = primary_ray(P, row, col, p.sq, disc[i]);
                        path_begin(p);
                        if (STATS) st.c[0]++;
                        mode = kFresh;
                    } else {
                        mode = kIdle;
                    }
                }
                next += (uint32_t)__popcll(freemask);
                if (next > N) next = N;
            }
            // --- (3) new segments: analytic shapes first (they bound the traversal), then start at the root
            if (mode == kFresh) {
                if (STATS) st.c[1]++;
                hit_rec = -1;
                tb = 0.0;
                scan_shapes_fast(P, p.r, p.self, hit_rec, tb);
                best = hit_rec >= 0 ? 0 : -1;  // triangle ids follow every shape id: a shape wins any tie
                bslot = -1;
                tb32 = hit_rec >= 0 ? upper32(tb) : 3.0e38f;
                trav_setup(P, p.r, T);
                trav_setup_q(P, T, TQ);
                cur = 0;
                sp = 0;
                mode = kTrav;
            }
            if (!any64(mode == kTrav)) break;  // after (1)-(3) a lane is traversing or idle
            // --- (4) traversal until enough lanes are ready to be shaded
            for (;;) {
                // inner nodes: every descending lane steps until the lanes that already hold a leaf outnumber the ones still
                // descending (then the leaf tests run for the majority instead of everybody waiting for the slowest lane).
                // One wave-uniform exit condition, evaluated on the scalar unit.
                for (;;) {
                    // a lane that is not traversing holds cur == kTravDone, so `cur` alone tells the three cases apart:
                    // >= 0 inner node, kTravDone nothing, any other negative value a leaf reference (one compare per ballot)
                    const bool inner = cur >= 0;
                    const int n_inner = __builtin_popcountll(__builtin_amdgcn_ballot_w64(inner));
                    const int n_leaf = __builtin_popcountll(__builtin_amdgcn_ballot_w64((uint32_t)cur > (uint32_t)kTravDone));
                    if (n_inner == 0 || n_leaf * FLUX_BVH_LEAF_NUM > n_inner * FLUX_BVH_LEAF_DEN) break;
                    if (inner) {
                    // 32-B node on the 16-bit grid: two 16-B gathers (the state machine is bound by their NUMBER); uniform
                    // base + 32-bit byte offset (abi.hip checks nodes * 32 < 2^32)
                    FLUX_TRIP_LANES(P, 12);
                    const uint4 *nq = reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(P.nodesq) + ((uint32_t)cur << 5));
                    const uint4 w0 = nq[0], w1 = nq[1];
                    struct { int child0, child1; } Nd = {(int)w1.z, (int)w1.w};
                    if (STATS) st.c[8]++;
                    float tn0, tn1;
                    // lo0 = (w0.x lo16, w0.x hi16, w0.y lo16)  hi0 = (w0.y hi16, w0.z lo16, w0.z hi16)
                    // lo1 = (w0.w lo16, w0.w hi16, w1.x lo16)  hi1 = (w1.x hi16, w1.y lo16, w1.y hi16)
                    const bool h0 = box_hit_q((float)(w0.x & 0xffffu), (float)(w0.x >> 16), (float)(w0.y & 0xffffu),
                                              (float)(w0.y >> 16), (float)(w0.z & 0xffffu), (float)(w0.z >> 16), TQ, tb32, tn0);
                    const bool h1 = box_hit_q((float)(w0.w & 0xffffu), (float)(w0.w >> 16), (float)(w1.x & 0xffffu),
                                              (float)(w1.x >> 16), (float)(w1.y & 0xffffu), (float)(w1.y >> 16), TQ, tb32, tn1);
                    int nxt;
                    if (h0 && h1) {
                        const bool near0 = tn0 <= tn1;
                        *reinterpret_cast<int *>(tstack + sp) = near0 ? Nd.child1 : Nd.child0;
                        sp += kEntry;
                        nxt = near0 ? Nd.child0 : Nd.child1;
                    } else if (h0) {
                        nxt = Nd.child0;
                    } else if (h1) {
                        nxt = Nd.child1;
                    } else if (sp > 0) {
                        sp -= kEntry;
                        nxt = *reinterpret_cast<const int *>(tstack + sp);
                    } else {
                        nxt = kTravDone;
                    }
                    cur = nxt;
                    }
                }
                if (mode == kTrav && cur < 0 && cur != kTravDone) {  // a lane holding a leaf: ~((first << 3) | count)
                    const int ref = ~cur;
                    const int first = ref >> 3, cnt = ref & 7;
                    for (int k = 0; k < cnt; ++k) {
                        double t;
                        FLUX_TRIP_LANES(P, 14);
                        if (STATS) st.c[9]++;
                        // uniform base + 32-bit byte offset (abi.hip checks triangles * sizeof(DevTri) < 2^32)
                        const DevTri &Tk = *reinterpret_cast<const DevTri *>(reinterpret_cast<const char *>(P.tris) +
                                                                             (uint32_t)(first + k) * (uint32_t)sizeof(DevTri));
                        if (tri_hit(Tk, p.r, t)) consider(t, Tk.id, first + k, best, bslot, tb);
                    }
                    if (best >= 0) tb32 = upper32(tb);
                    if (sp > 0) {
                        sp -= kEntry;
                        cur = *reinterpret_cast<const int *>(tstack + sp);
                    } else {
                        cur = kTravDone;
                    }
                }
                if (mode == kTrav && cur == kTravDone) mode = kShade;
                const int n_trav = __popcll(ballot64(mode == kTrav));
                const int n_ready = __popcll(ballot64(mode == kShade));
                if (n_trav == 0 || n_ready >= FLUX_BVH_REFILL_AT) break;
            }
        }
    }
    finish_pixel(P, wave_on, lane, 0u, 64u, pixel, sr, sg, sb);
    flush_stats<STATS>(P, st, lane);
}


// ---------------------------------------------------------------------------
// BVH variant over the 4-WIDE tree (flux_bvh.h DevNode4Q / DevLeafRec; the default for FAST mesh scenes).
// Same state machine as render_bvh_kernel -- persistent lanes, leaf vote, refill threshold --, another memory layout.
// Measured on the binary kernel (profiles/r03_experiments/pmcmem_r03a_*.log): the CU's texture-data path is 98 % busy, the
// address unit 71 %, the VALU 72 %: the kernel is bound by the vector-memory pipeline, whose cost is per active lane and
// per 128-B LINE filled (scripts/micro/gather_rate.hip: ~2.4 cycles per lane-line from the L2, ~9 from beyond it, ~0.4
// for a further 16-B piece of the same line).  So:
//   * a visit fetches ONE 64-B node = the boxes of four children (half a line, four pieces) and the tree is half as deep;
//   * a leaf is ONE 128-B record that holds both halves of a quad (tri A = v0,e1,e2, tri B = v0,e2,e3; the operands of the
//     DevTri records bit for bit, so the exact f64 test and its results are unchanged); triangles that do not pair up
//     get a record each;
//   * the slab test needs no per-plane min/max: the ray's direction signs say which of lo | hi is the near plane (box_hit4:
//     a per-lane v_perm selector, or a rotate by 0 / 16 in the form without v_perm, measured slower) -- the boxes of an empty slot
//     (lo 65535, hi 0) then fail by themselves.
// The nearest hit child is singled out by three compare-exchanges on (t_near, link) and entered; the others are stacked
// as they come (fully sorted, five exchanges, was measured: 0.6 % fewer visits, 3.7 % more time).  A pixel's camera
// rays start at pixel_entry_node instead of the root.  The node loop is left for the leaf step by the leaf vote, and for
// the shading step once FLUX_BVH4_EARLY_AT walks have ended.  Hit selection is the brute-force rule, so everything the
// tests say of render_bvh_kernel holds here.
// ---------------------------------------------------------------------------
// Slab test without conversions or min/max: float(2^23 + q) is the bit pattern 0x4B000000 | q, so ONE v_perm_b32 per plane
// builds it from the packed lo | hi << 16 word -- its per-lane byte selector also picks WHICH half is the near plane (the
// ray's direction sign), so no rotate is needed -- and the 2^23 folds into the plane constant:
//     t = (2^23 + q) s + (c - 2^23 s).
// The near and far planes of an axis go through one packed v_pk_fma_f32.  c - 2^23 s is rounded once (<= |s| / 2, half a
// grid quantum in t) and then moved one more quantum outward, so the test stays conservative (boxes are in effect padded
// by at most 1.5 quanta more, ~1e-4 of a triangle's size on the 1 M-triangle mesh).
struct TravRay4 {
    // step / d of the three axes.  v_pk_fma_f32 reads a 64-bit register pair per operand and picks, per result half, which
    // half of the pair it takes (op_sel / op_sel_hi): a splat (s, s) therefore needs ONE register, as long as the pair's
    // other half holds something useful -- (sx, sy) share a pair, sz shares one with whatever the compiler puts beside it
    flux_f2 sxy;
    flux_f2 szt;               // (sz, tb32): the z step beside the f32 upper bound of the best hit distance so far
    flux_f2 cx, cy, cz;        // (near constant, far constant), 2^23 s folded in
    uint32_t nx, ny, nz;       // v_perm selectors of the near plane's half ...
    uint32_t fx, fy, fz;       // ... and the far plane's
};
__device__ __forceinline__ void trav_setup4(const RenderParams &P, const TravRay &T, TravRay4 &Q) {
    const float lox = __builtin_fmaf(P.bvh_qmin[0], T.ix, T.lox), hix = __builtin_fmaf(P.bvh_qmin[0], T.ix, T.hix);
    const float loy = __builtin_fmaf(P.bvh_qmin[1], T.iy, T.loy), hiy = __builtin_fmaf(P.bvh_qmin[1], T.iy, T.hiy);
    const float loz = __builtin_fmaf(P.bvh_qmin[2], T.iz, T.loz), hiz = __builtin_fmaf(P.bvh_qmin[2], T.iz, T.hiz);
    const bool ngx = T.ix < 0.0f, ngy = T.iy < 0.0f, ngz = T.iz < 0.0f;  // 1/d is never 0 (trav_setup)
    const float sx = P.bvh_qstep[0] * T.ix, sy = P.bvh_qstep[1] * T.iy, sz = P.bvh_qstep[2] * T.iz;
    constexpr float k23 = 8388608.0f;
    constexpr uint32_t kLoHalf = 0x07060100u, kHiHalf = 0x07060302u;  // bytes 7,6 of {K, w} = 0x4B00; then w's low / high half
    Q.sxy = flux_f2{sx, sy};
    Q.szt[0] = sz;
    Q.cx = flux_f2{__builtin_fmaf(-k23, sx, ngx ? hix : lox) - fabsf(sx), __builtin_fmaf(-k23, sx, ngx ? lox : hix) + fabsf(sx)};
    Q.cy = flux_f2{__builtin_fmaf(-k23, sy, ngy ? hiy : loy) - fabsf(sy), __builtin_fmaf(-k23, sy, ngy ? loy : hiy) + fabsf(sy)};
    Q.cz = flux_f2{__builtin_fmaf(-k23, sz, ngz ? hiz : loz) - fabsf(sz), __builtin_fmaf(-k23, sz, ngz ? loz : hiz) + fabsf(sz)};
    Q.nx = ngx ? kHiHalf : kLoHalf;  Q.fx = ngx ? kLoHalf : kHiHalf;
    Q.ny = ngy ? kHiHalf : kLoHalf;  Q.fy = ngy ? kLoHalf : kHiHalf;
    Q.nz = ngz ? kHiHalf : kLoHalf;  Q.fz = ngz ? kLoHalf : kHiHalf;
}
// The splats (s, s) are written as shuffles of the pairs: v_pk_fma_f32 picks, per result half, which half of an operand's
// register pair it reads (op_sel / op_sel_hi), so a splat costs no register -- as long as the shuffle stays next to the
// fma.  Hoisted out of the node loop it would be materialised in two registers per axis; render_bvh4_kernel therefore
// passes the pairs through an empty asm inside the loop (trav_pin4), which pins them where they are and costs nothing.
// (NOT volatile: a volatile asm counts as a possible store, and every wave-uniform load after it -- the scene records of
// scan_shapes_fast, read with scalar loads -- would become a vector load; the node index as an input keeps it in the loop)
__device__ __forceinline__ void trav_pin4(TravRay4 &Q, int cur) { asm("" : "+v"(Q.sxy), "+v"(Q.szt) : "v"(cur)); }
__device__ __forceinline__ bool box_hit4(uint32_t wx, uint32_t wy, uint32_t wz, const TravRay4 &Q, float tb32, float &tnear) {
    constexpr uint32_t K = 0x4B000000u;
    const flux_f2 qx = {__uint_as_float(__builtin_amdgcn_perm(K, wx, Q.nx)), __uint_as_float(__builtin_amdgcn_perm(K, wx, Q.fx))};
    const flux_f2 qy = {__uint_as_float(__builtin_amdgcn_perm(K, wy, Q.ny)), __uint_as_float(__builtin_amdgcn_perm(K, wy, Q.fy))};
    const flux_f2 qz = {__uint_as_float(__builtin_amdgcn_perm(K, wz, Q.nz)), __uint_as_float(__builtin_amdgcn_perm(K, wz, Q.fz))};
    const flux_f2 tx = __builtin_elementwise_fma(qx, __builtin_shufflevector(Q.sxy, Q.sxy, 0, 0), Q.cx);
    const flux_f2 ty = __builtin_elementwise_fma(qy, __builtin_shufflevector(Q.sxy, Q.sxy, 1, 1), Q.cy);
    const flux_f2 tz = __builtin_elementwise_fma(qz, __builtin_shufflevector(Q.szt, Q.szt, 0, 0), Q.cz);
    const float tn = fmaxf(fmaxf(tx[0], ty[0]), tz[0]);
    const float tf = fminf(fminf(tx[1], ty[1]), tz[1]);
    tnear = tn;
    return fmaxf(tn, 0.0f) <= fminf(tf, tb32);  // tn <= tf, tf >= 0, tn <= tb32 (tb32 > 0)
}

// The stack bound (BvhInfo::wide_stack) counts the OCCUPIED slots of a node, so an empty slot (lo 65535, hi 0 on every axis,
// link kTravDone) must never be stacked.  Its inverted box fails the slab test by itself as long as the ray's padding
// (trav_setup: 2^-20 (bvh_mag + |o|)) is small against the grid; a ray whose padding exceeds the WHOLE grid on every axis --
// a mesh of 1e-4 seen from hundreds of units away, or placed at coordinates 1e6 times its size, or a ray with a NaN in it --
// passes every box, empty ones too.  Whether it does is a property of the ray alone (the empty slot's words are the same in
// every node and the test is deterministic), so it is decided ONCE per ray, by running the test itself on those words with
// no bound on t.  For such a ray the slab test carries no information anyway (a box that contains another passes whenever
// the inner one does, and every occupied box lies inside the grid), so its constants are replaced by ones under which the
// test reads "lo.x <= hi.x" -- true for every occupied box (bvh.cpp quantize_bvh verifies lo <= hi), false for an empty slot:
// t_near = 2^-100 lo.x, t_far = 2^-100 hi.x, both exact, far below any hit distance (t > T_MIN).  The walk then visits every
// node and leaf in stack order and the exact f64 test decides, as always.  Nothing changes per node visit.
__device__ __forceinline__ void trav_guard4(TravRay4 &Q) {
    float t_;
    if (box_hit4(0x0000ffffu, 0x0000ffffu, 0x0000ffffu, Q, 3.0e38f, t_)) {
        constexpr float kEps = 7.8886090522101181e-31f;  // 2^-100
        Q.sxy = flux_f2{kEps, 0.0f};
        Q.szt[0] = 0.0f;
        Q.cx = flux_f2{-kEps * 8388608.0f, -kEps * 8388608.0f};
        Q.nx = 0x07060100u;  // lo half near, hi half far
        Q.fx = 0x07060302u;
        Q.cy = Q.cz = flux_f2{-3.0e38f, 3.0e38f};
    }
}

// Where a pixel's camera rays enter the 4-wide tree.  All of a pixel's primary rays lie in one thin bundle: origins on the
// lens (within the square of side 2 lens_radius around the eye), passing through the pixel's footprint F on the focal plane
// (primary_ray: o + d = e + u factor U + v factor V - focal W does not depend on the lens point).  A point of the bundle is
// (1 - t) o + t f, t >= 0, so per axis it lies between two LINEAR bounds on t in [0, 1] and two others on t >= 1.  A box
// that no such point can reach (tested per axis, boxes widened by two grid quanta: ~3e-5 of the mesh, eleven orders
// above the f64 rounding of primary_ray) holds no triangle any ray of the bundle can hit, so the walk from the root
// may skip it for ALL of them: descend while exactly one child can be reached, and start every camera ray of the pixel at
// the node (or leaf) where that stops.  The nearest hit is the brute-force one either way; only visits are saved.
// One wave per pixel: lane = child (0..3) + 4 * t-range (0..1); ~10 levels once per pixel against thousands of segments.
__device__ __forceinline__ int pixel_entry_node(const RenderParams &P, int row, int col, uint32_t lane) {
    const double qs[3] = {(double)P.bvh_qstep[0], (double)P.bvh_qstep[1], (double)P.bvh_qstep[2]};
    const double qm[3] = {(double)P.bvh_qmin[0], (double)P.bvh_qmin[1], (double)P.bvh_qmin[2]};
    const double U[3] = {P.Ux, P.Uy, P.Uz}, V[3] = {P.Vx, P.Vy, P.Vz}, W[3] = {P.Wx, P.Wy, P.Wz}, E[3] = {P.ex, P.ey, P.ez};
    const double ua = P.aps * ((double)col - P.half_w) * P.factor, ub = P.aps * (((double)col - P.half_w) + 1.0) * P.factor;
    const double va = P.aps * ((double)(P.img_h - row) - P.half_h) * P.factor,
                 vb = P.aps * (((double)(P.img_h - row) - P.half_h) + 1.0) * P.factor;
    const double R = fabs(P.lens_radius);
    const uint32_t c = lane & 3u;
    const bool far_range = (lane & 4u) != 0u;  // t >= 1: beyond the focal plane
    double Lo[3], Ls[3], Uo[3], Us[3];  // lower bound Lo + t Ls, upper bound Uo + t Us of the bundle's points
    double mag = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double fc = E[a] - P.focal * W[a];
        const double f_lo = fc + fmin(ua * U[a], ub * U[a]) + fmin(va * V[a], vb * V[a]);
        const double f_hi = fc + fmax(ua * U[a], ub * U[a]) + fmax(va * V[a], vb * V[a]);
        const double ro = R * (fabs(U[a]) + fabs(V[a]));
        const double omin = E[a] - ro, omax = E[a] + ro;
        Lo[a] = far_range ? omax : omin;
        Uo[a] = far_range ? omin : omax;
        Ls[a] = f_lo - Lo[a];
        Us[a] = f_hi - Uo[a];
        mag = fmax(mag, fmax(fabs(omin), fabs(omax)));
        mag = fmax(mag, fmax(fabs(f_lo), fabs(f_hi)));
    }
    // the two quanta must dwarf f64 rounding at the bundle's coordinates; a camera 1e9 mesh extents away starts at the root
    if (!(mag * 1e-9 < fmin(qs[0], fmin(qs[1], qs[2])))) return 0;
    int node = 0;
    for (int level = 0; level < 64; ++level) {
        const uint32_t *nq = reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(P.nodes4) + ((uint32_t)node << 6));
        const uint32_t w[3] = {nq[c], nq[4 + c], nq[8 + c]};
        const int link = wide_link(nq[12], c);  // arithmetic on the node's meta word (flux_bvh.h); an empty slot's box is inverted
        double tl = far_range ? 1.0 : 0.0, th = far_range ? 1.0e300 : 1.0;
        bool ok = (w[0] & 0xffffu) <= (w[0] >> 16) && lane < 8u;
        for (int a = 0; a < 3; ++a) {
            const double lo = fma((double)(w[a] & 0xffffu), qs[a], qm[a]) - 2.0 * qs[a];
            const double hi = fma((double)(w[a] >> 16), qs[a], qm[a]) + 2.0 * qs[a];
            const double c1 = hi - Lo[a];  // Lo + t Ls <= hi
            if (Ls[a] > 0.0) th = fmin(th, c1 / Ls[a]);
            else if (Ls[a] < 0.0) tl = fmax(tl, c1 / Ls[a]);
            else ok = ok && c1 >= 0.0;
            const double c2 = lo - Uo[a];  // Uo + t Us >= lo
            if (Us[a] > 0.0) tl = fmax(tl, c2 / Us[a]);
            else if (Us[a] < 0.0) th = fmin(th, c2 / Us[a]);
            else ok = ok && c2 <= 0.0;
        }
        // (a quotient is rounded by 1e-16 of itself; the two quanta on the box move it by ~1e-5: no further margin)
        const unsigned long long m8 = ballot64(ok && tl <= th);
        const uint32_t m = (uint32_t)__builtin_amdgcn_readfirstlane((int)(((uint32_t)m8 | (uint32_t)(m8 >> 4)) & 15u));
        if (m == 0u) return kTravDone;            // the bundle misses the mesh
        if ((m & (m - 1u)) != 0u) return node;    // two children or more can be reached: start here
        const int next = __builtin_amdgcn_readlane(link, (int)__builtin_ctz(m));
        if (next < 0) return next;                // a leaf reference
        node = next;
    }
    return node;
}

template <bool STATS, bool LDS_SCENE, bool TYP>
__global__ __launch_bounds__(FLUX_BLOCK_THREADS, FLUX_WPE_BVH4) void render_bvh4_kernel(const RenderParams P0) {
    const RenderParams &P = P0;  // outside the pass loop; inside it is shadowed by the reloaded view
    extern __shared__ double lds_stack[];
    const int tid = threadIdx.x;  // one wave per block (launch plan)
    const uint32_t lane = tid & 63;
    // traversal stack [entry][lane] in LDS; `sp` is the ADDRESS of the lane's next free entry (+-256 per entry: no index
    // arithmetic per push / pop), the stack is empty when sp == sp0
    char *const sp0 = reinterpret_cast<char *>(lds_stack) + tid * 4;
    constexpr int kEntry = 64 * 4;
    // the analytic scene's hit records, the materials and the scan spheres behind the stack (as in render_split_kernel): the shading
    // step's dependent gathers -- triangle record -> material record, hit record, a sphere record per candidate -- lose an L2 round trip
    // (LDS_SCENE: the launch plan chose this instantiation and reserved the bytes -- small analytic sets only, plan_render)
    const char *const frec_lds = reinterpret_cast<const char *>(lds_stack) + (size_t)(P.bvh4_stack > 0 ? P.bvh4_stack : 1) * kEntry;
    const int n_rec = TYP ? P.n_sph + P.n_pln + P.n_dsk : hit_records(P);  // (TYP: a scene without boxes)
    const char *const mats_lds = frec_lds + (size_t)n_rec * sizeof(DevHitRec);
    const char *const fsph_lds = mats_lds + (size_t)P.n_mats * sizeof(DevMaterial);
    if constexpr (LDS_SCENE) {
        uint32_t *dst = reinterpret_cast<uint32_t *>(const_cast<char *>(frec_lds));
        const uint32_t n1 = (uint32_t)n_rec * (uint32_t)(sizeof(DevHitRec) / 4), n2 = (uint32_t)P.n_mats * (uint32_t)(sizeof(DevMaterial) / 4),
                       n3 = (uint32_t)P.n_sph * 8u;
        const uint32_t *s1 = reinterpret_cast<const uint32_t *>(P.frec), *s2 = reinterpret_cast<const uint32_t *>(P.mats),
                       *s3 = reinterpret_cast<const uint32_t *>(P.fsph);
        for (uint32_t w = (uint32_t)tid; w < n1; w += 64u) dst[w] = s1[w];
        for (uint32_t w = (uint32_t)tid; w < n2; w += 64u) dst[n1 + w] = s2[w];
        for (uint32_t w = (uint32_t)tid; w < n3; w += 64u) dst[n1 + n2 + w] = s3[w];
        __syncthreads();
    }

    const uint32_t N = P.nsamp;
    const uint64_t wave = blockIdx.x;
    int lrow = 0, col = 0, row = 0;
    uint32_t set = 0;
    uint64_t pixel = 0;
    const bool wave_on = map_wave(P, wave, lrow, col, row, set, pixel);  // wave-uniform
    set = (uint32_t)__builtin_amdgcn_readfirstlane((int)set);
    col = __builtin_amdgcn_readfirstlane(col);
    row = __builtin_amdgcn_readfirstlane(row);

    Stats st = {};
    // the pixel's sum is kept PER WAVE, not per lane: the radiance of the paths that end in a pass is
    // added over the wave at once (wave_sum1's fixed tree; lanes without an ended path contribute 0) and the totals live in
    // scalar registers -- six vector registers less per lane, for ~75 instructions per shading pass.  The order of the additions
    // follows the wave's own schedule, which depends on nothing but the scene and the samples: bit-reproducible, independent of
    // the sharding.  0: per-lane sums (the compiler then spills 35 vector registers at 5 waves/SIMD).
    double tot_r = 0.0, tot_g = 0.0, tot_b = 0.0;
    const auto uniform64 = [](double x) {
        return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(x)), __builtin_amdgcn_readfirstlane(__double2loint(x)));
    };
    if (wave_on) {
        const double2 *pix = P.pix + (size_t)set * N;
        const double2 *disc = P.disc + (size_t)set * N;
        // the pixel's constants of primary_ray, wave-uniform: kept in scalar registers (ten vector registers otherwise)
        const PixelConsts PX = pixel_consts(P, row, col);

        enum { kIdle = 0, kWant = 1, kFresh = 2, kTrav = 3, kShade = 4 };
        int mode = kWant;
        uint32_t next = 0;  // wave-uniform cursor: first unstarted sample
        uint32_t i = 0;
        Path p;
        path_begin(p);
        p.sq = make_double2(0.0, 0.0);
        p.r = Ray{0, 0, 0, 0, 0, 1};
        TravRay4 TQ = {};
        TQ.szt[1] = 3.0e38f;
        int cur = kTravDone;
        char *sp = sp0;
        uint32_t top = 0u;  // the top stack entry, in a register: meta word | mask of the pending slots; 0 = the stack is empty
#ifdef FLUX_DEBUG_DEADEND
        bool popped_ = false;  // the node in `cur` came off the stack (not entered as the nearest child)
#endif
        // the nearest hit so far in ONE register: -1 none, >= 0 a triangle (its slot in leaf order), <= -2 an analytic shape
        // (-2 - hit record).  The tie rule (equal t keeps the lower hit-order index, scene.rs:156-160) needs the index of the
        // current best only when two distances are EQUAL: it is fetched then (consider4), not carried.
        int win = -1;
        double tb = 0.0;
        // the path's bounce weights as the material indices of its bounces, mat_bits each (the launch plan picks this kernel
        // only if (max_trace_depth - 1) mat_bits <= 32): FAST's weights f (n.wi)/pdf are constants of the material (closed
        // form), so the throughput is multiplied up from the weight table when the path ENDS -- the same products in the same
        // order as a running product, in one register instead of six
        // (a list of the bounces' materials instead of the running product was measured: its gathers cost more than its registers buy)
        uint32_t mlist = 0u;
        const uint32_t mat_bits = (uint32_t)P.mat_bits, mat_mask = (1u << mat_bits) - 1u;
        (void)mlist;
        (void)mat_mask;
        const auto consider4 = [&](double t, int id, int slot) {
            bool take = win == -1 || t < tb;
            if (!take && t == tb && win >= 0)
                take = id < reinterpret_cast<const DevTri *>(reinterpret_cast<const char *>(P.tris) + (uint32_t)win * (uint32_t)sizeof(DevTri))->id;
            if (take) {
                win = slot;
                tb = t;
            }
        };
        const int entry = pixel_entry_node(P, row, col, lane);  // wave-uniform
        for (;;) {
            // The kernel arguments are read afresh in every pass (scalar loads from the kernarg segment, served by the scalar
            // cache): handed the plain by-value struct the compiler loads every field it will ever need ONCE, keeps ~170 scalar
            // registers' worth alive across the whole loop and spills the excess into vector-register lanes -- a v_readlane
            // (a VALU slot) per use.  The empty asm makes the pointer a new value per pass (its input, the sample cursor, changes),
            // so loads cannot move above it.
            const RenderParams &P = relaunder_params(next);
            // --- (1) Scene::shade after the hit, for the lanes whose traversal is complete
            double Lr = 0.0, Lg = 0.0, Lb = 0.0;  // what the path that ended in this pass adds to the pixel (0: none ended)
            if (mode == kShade) {
                FLUX_TRIP_LANES(P, 10);
                bool cont = shade_hit<STATS, true, false, LDS_SCENE, TYP>(P, p, set, i, win >= 0 ? 0 : -2 - win, win >= 0 ? win : -1, tb, nullptr, 0,
                                                                     Lr, Lg, Lb, st, 0, frec_lds, mats_lds);
                if (cont && p.depth > P.max_depth) {  // scene.rs:164-165 on entry to the next level
                    cont = false;
                    Lr = Lg = Lb = 0.0;
                    if (STATS) st.c[7]++;
                } else if (cont) {
                }
                if (cont) {
                    mode = kFresh;
                } else {
                    // fold_path: L * prod_k weight[material of bounce k], front to back (materials.rs:31-33, 69-71 in closed form)
                    fold_path(p, nullptr, 0, Lr, Lg, Lb);  // the running product (six registers)
                    mode = kWant;
                }
            }
            if (any64(mode == kWant)) {  // trace.rs:82, for the whole wave at once (only lanes that just ended a path are in kWant here)
                tot_r = uniform64(tot_r + wave_sum1(Lr));
                tot_g = uniform64(tot_g + wave_sum1(Lg));
                tot_b = uniform64(tot_b + wave_sum1(Lb));
            }
            // --- (2) compaction: hand the pixel's next samples to the free lanes (ballot + mbcnt prefix)
            const unsigned long long freemask = ballot64(mode == kWant);
            if (freemask) {
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(freemask >> 32),
                                                                __builtin_amdgcn_mbcnt_lo((uint32_t)freemask, 0u));
                if (mode == kWant) {
                    i = next + rank;
                    if (i < N) {
                        p.sq = pix[i];
                        p.r = primary_ray_px(P, PX, p.sq, disc[i]);
                        path_begin(p);
                        mlist = 0u;
                        if (STATS) st.c[0]++;
                        mode = kFresh;
                    } else {
                        mode = kIdle;
                    }
                }
                next += (uint32_t)__popcll(freemask);
                if (next > N) next = N;
            }
            // --- (3) new segments: analytic shapes first (they bound the traversal), then start at the root
            if (mode == kFresh) {
                if (STATS) st.c[1]++;
                int hit_rec = -1;
                tb = 0.0;
                scan_shapes_fast<false, LDS_SCENE, TYP, TYP>(P, p.r, p.self, hit_rec, tb, nullptr, fsph_lds);  // (TYP: at most 32 spheres too)
                win = hit_rec >= 0 ? -2 - hit_rec : -1;  // triangle ids follow every shape id: a shape wins any tie
                TQ.szt[1] = hit_rec >= 0 ? upper32(tb) : 3.0e38f;
                TravRay T;
                trav_setup(P, p.r, T);
                trav_setup4(P, T, TQ);
                trav_guard4(TQ);
                cur = p.depth == 1 ? entry : 0;  // a camera ray starts below the part of the tree its pixel's bundle cannot touch
                sp = sp0;
                top = 0u;
                mode = kTrav;
            }
            if (!any64(mode == kTrav)) break;  // after (1)-(3) a lane is traversing or idle
            // the arena's base, read ONCE per pass: through the re-read view of the kernel arguments (a generic pointer) the
            // compiler cannot tell that the stack's LDS writes leave it alone and fetched it again in every node and leaf step --
            // a scalar load and a wait in front of every node fetch
            const char *const arena = reinterpret_cast<const char *>(P.nodes4);
            const int n_busy_max = 64 - __builtin_popcountll(__builtin_amdgcn_ballot_w64(mode == kIdle));  // lanes that still have work
            // --- (4) traversal until enough lanes are ready to be shaded
            for (;;) {
                bool refill_now = false;
                for (;;) {  // inner nodes, with the leaf vote of render_bvh_kernel
                    const bool inner = cur >= 0;
                    const int n_inner = __builtin_popcountll(__builtin_amdgcn_ballot_w64(inner));
                    const int n_leaf = __builtin_popcountll(__builtin_amdgcn_ballot_w64((uint32_t)cur > (uint32_t)kTravDone));
                    // lanes whose walk has ended since the last leaf step are not marked yet: once the refill threshold is reached
                    // among them the wave leaves for the shading step at once instead of stepping on for the few still descending
                    // (lanes that hold a leaf keep it: `cur` is persistent state)
                    if (n_busy_max - n_inner - n_leaf >= FLUX_BVH4_EARLY_AT) {
                        refill_now = true;
                        break;
                    }
                    if (n_inner == 0 || n_leaf * FLUX_BVH_LEAF_NUM > n_inner * FLUX_BVH_LEAF_DEN) break;
#if defined(FLUX_DEBUG_TRIPS) && defined(FLUX_DEBUG_WAIT)  // experiment builds (scripts/bvh_wait_census.py): what the lanes that are NOT traversing wait for
                    {
                        const int n_done_ = __builtin_popcountll(__builtin_amdgcn_ballot_w64(mode == kShade));
                        if (P.stats && lane == 0) {
                            atomicAdd(P.stats + 14, (unsigned long long)n_leaf);
                            atomicAdd(P.stats + 15, (unsigned long long)n_done_);
                        }
                    }
#endif
                    if (inner) {
                        // ONE stack entry per node (flux_bvh.h DevNode4A): the node's meta word with the mask of the hit children
                        // that are not entered now.  The nearest hit child is entered, a pop takes the entry's lowest pending slot;
                        // either way the link is arithmetic on (entry, slot) -- a node's children are contiguous in the arena.
                        FLUX_TRIP_LANES(P, 12);
                        const char *nb = arena + ((uint32_t)cur << 6);
                        const uint4 *nq = reinterpret_cast<const uint4 *>(nb);
                        const uint4 bx = nq[0], by = nq[1], bz = nq[2];
                        const uint32_t meta = *reinterpret_cast<const uint32_t *>(nb + 48);
                        if (STATS) st.c[8]++;
                        const float kFar = 3.0e38f;
                        float t0, t1, t2, t3;
                        trav_pin4(TQ, cur);
                        const bool h0 = box_hit4(bx.x, by.x, bz.x, TQ, TQ.szt[1], t0);
                        const bool h1 = box_hit4(bx.y, by.y, bz.y, TQ, TQ.szt[1], t1);
                        const bool h2 = box_hit4(bx.z, by.z, bz.z, TQ, TQ.szt[1], t2);
                        const bool h3 = box_hit4(bx.w, by.w, bz.w, TQ, TQ.szt[1], t3);
                        // (an empty slot's inverted box always fails the test -- trav_guard4 sees to it per ray --, so it never
                        // gets a mask bit and the stack bound BvhInfo::wide_stack, one entry per node with two children, holds)
                        float k0 = h0 ? t0 : kFar, k1 = h1 ? t1 : kFar, k2 = h2 ? t2 : kFar, k3 = h3 ? t3 : kFar;
                        asm("" : "+v"(k0), "+v"(k1), "+v"(k2), "+v"(k3));
                        // the mask of the hit slots, from the slab tests' own verdicts
                        const uint32_t hm = (h0 ? 1u : 0u) | (h1 ? 2u : 0u) | (h2 ? 4u : 0u) | (h3 ? 8u : 0u);
                        // the nearest hit slot: a tournament on the entry distances
                        const bool a01 = k1 < k0, a23 = k3 < k2;
                        const float m01 = a01 ? k1 : k0, m23 = a23 ? k3 : k2;
                        const uint32_t s01 = a01 ? 1u : 0u, s23 = a23 ? 3u : 2u;
                        const bool a = m23 < m01;
                        const uint32_t near_slot = a ? s23 : s01;
                        const bool hit = hm != 0u;
#ifdef FLUX_DEBUG_DEADEND  // experiment builds: node visits in which NO child box passes (slot 10) of all node visits (slot 11), and
                           // those dead ends that were reached by a pop (slot 12: `cur` came off the stack) -- stale entries
                        if (P.stats) {
                            const unsigned long long dead_ = ballot64(!hit), all_ = ballot64(true), pdead_ = ballot64(!hit && popped_);
                            if (__builtin_amdgcn_mbcnt_hi((uint32_t)(all_ >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)all_, 0u)) == 0) {
                                atomicAdd(P.stats + 10, (unsigned long long)__popcll(dead_));
                                atomicAdd(P.stats + 11, (unsigned long long)__popcll(all_));
                                atomicAdd(P.stats + 12, (unsigned long long)__popcll(pdead_));
                            }
                        }
                        popped_ = !hit;
#endif
                        // the child to go on with: the nearest hit slot of this node, else the lowest pending slot of the top entry
                        const uint32_t e = hit ? meta : top;
                        const uint32_t slot = hit ? near_slot : (uint32_t)(__ffs((int)top) - 1);
                        int nxt = wide_link(e, slot);
                        if (hit) {
                            const uint32_t pend = hm & ~(1u << near_slot);
                            if (pend != 0u) {  // ONE entry for all the other hit children; the previous top goes to LDS
                                if (top != 0u) {
                                    *reinterpret_cast<uint32_t *>(sp) = top;
                                    sp += kEntry;
                                }
                                top = meta | pend;
                            }
                        } else if (top != 0u) {
                            top &= top - 1u;  // (an entry's lowest set bit is a mask bit: its mask is never 0)
                            if ((top & 15u) == 0u) {  // exhausted: the entry below comes up NOW, its LDS latency behind the child's visit
                                top = 0u;
                                if (sp != sp0) {
                                    sp -= kEntry;
                                    top = *reinterpret_cast<const uint32_t *>(sp);
                                }
                            }
                        } else {
                            nxt = kTravDone;
                        }
                        cur = nxt;
                    }
                }
                if (
                    !refill_now &&
                    mode == kTrav && cur < 0 && cur != kTravDone) {  // a lane holding a leaf: ~(unit of its ONE record)
#ifndef FLUX_DEBUG_WAIT
                    FLUX_TRIP_LANES(P, 14);
#endif
                    const DevLeafRec &R = *reinterpret_cast<const DevLeafRec *>(arena + ((uint32_t)~cur << 6));
                    const V3 v0 = mk(R.v0[0], R.v0[1], R.v0[2]), e1 = mk(R.e1[0], R.e1[1], R.e1[2]), e2 = mk(R.e2[0], R.e2[1], R.e2[2]);
                    const int idA = R.id[0], idB = R.id[1], slA = R.slot[0], slB = R.slot[1];
                    double t;
                    if (STATS) st.c[9]++;
                    if (tri_hit_v(v0, e1, e2, p.r, t)) consider4(t, idA, slA);
                    if (slB >= 0) {  // the quad's other half: (v0, e2, e3)
                        const V3 e3 = mk(R.e3[0], R.e3[1], R.e3[2]);
                        if (STATS) st.c[9]++;
                        if (tri_hit_v(v0, e2, e3, p.r, t)) consider4(t, idB, slB);
                    }
                    if (win != -1) TQ.szt[1] = upper32(tb);
                    int nxt = wide_link(top, (uint32_t)(__ffs((int)top) - 1));
#ifdef FLUX_DEBUG_DEADEND
                    popped_ = true;
#endif
                    if (top != 0u) {
                        top &= top - 1u;
                        if ((top & 15u) == 0u) {
                            top = 0u;
                            if (sp != sp0) {
                                sp -= kEntry;
                                top = *reinterpret_cast<const uint32_t *>(sp);
                            }
                        }
                    } else {
                        nxt = kTravDone;
                    }
                    cur = nxt;
                }
                if (mode == kTrav && cur == kTravDone) mode = kShade;  // (wide_link never yields kTravDone: units stay below 2^26)
                const int n_trav = __popcll(ballot64(mode == kTrav));
                const int n_ready = __popcll(ballot64(mode == kShade));
                if (n_trav == 0 || n_ready >= FLUX_BVH_REFILL_AT) break;
            }
        }
    }
    finish_pixel(P, wave_on, lane, 0u, 64u, pixel, lane == 0u ? tot_r : 0.0, lane == 0u ? tot_g : 0.0, lane == 0u ? tot_b : 0.0);
    flush_stats<STATS>(P, st, lane);
}

#endif  // FLUX_FAST

// ---- Scene::shade for caller-supplied rays (flux_debug_shade): one lane = one ray, traced from `depth`
// with sample (set, index) exactly as the render loop would; also reports the first hit (YAML shape index, or
// num_shapes + triangle id, or -1) and its distance.  Test hook: ray-level parity incl. the reference's quirks.
template <bool TRIS>
__global__ __launch_bounds__(64, 1) void shade_rays_kernel(const RenderParams P, const double *rays, int n, int depth,
                                                          uint32_t set, uint32_t index, double *out_rgb, int *out_hit,
                                                          double *out_t) {
    extern __shared__ double lds_stack[];
    const int tid = threadIdx.x;
    const int k = blockIdx.x * 64 + tid;
    double *stk = lds_stack + tid;
    int *tstack = bvh_stack_base(lds_stack, P, 64) + tid;
    if (k >= n) return;
    Stats st = {};
    Path p;
    path_begin(p);
    p.depth = depth;
    p.sq = P.pix[(size_t)set * P.nsamp + index];
    p.r = Ray{rays[6 * k], rays[6 * k + 1], rays[6 * k + 2], rays[6 * k + 3], rays[6 * k + 4], rays[6 * k + 5]};
    {   // first hit, reported in the reference's numbering
        double t = 0.0;
        int slot = -1;
        const int hit = scene_hit<false, TRIS>(P, p.r, path_self(p), t, slot, tstack, 64, st);
        int id = hit;
#if FLUX_FAST
        if (hit >= 0 && !(TRIS && slot >= 0)) id = P.frec[hit].orig_id;
#endif
        out_hit[k] = id;
        out_t[k] = hit >= 0 ? t : 0.0;
    }
    double Lr, Lg, Lb;
    while (shade_level<false, TRIS>(P, p, set, index, stk, 64, tstack, Lr, Lg, Lb, st)) {
    }
    fold_path(p, stk, 64, Lr, Lg, Lb);
    out_rgb[3 * k] = Lr;
    out_rgb[3 * k + 1] = Lg;
    out_rgb[3 * k + 2] = Lb;
}

// This copy of the bodies, as kernel_exists (flux_plan.h) names it
constexpr KernelCopy kThisCopy = !FLUX_FAST ? kCopyStrict : FLUX_DIEL ? kCopyFastDiel : kCopyFast;

// Runs the render kernel the launch plan names (launch_plan.cpp plan_render).  Nothing is decided here: the plan's fields become
// template arguments -- all of them as ONE compile-time constant (with_const, render.hip) -- and kernel arguments, and each kernel is
// named once, behind kernel_exists' word (flux_plan.h) that this copy compiles it with those arguments.  A plan that names another
// is hipErrorInvalidValue before anything is launched.  `p.stats` is a property of the call, not of the plan.
static hipError_t launch_render_impl(const LaunchPlan &L, const RenderParams &p, hipStream_t stream) {
    if (L.blocks > 0x7fffffffull || !plan_exists(kPassRender, L)) return hipErrorInvalidValue;
    const dim3 g((unsigned)L.blocks), b(L.block);
    const size_t lds = L.lds;
    RenderParams ps = p;  // the split kernel's
    ps.tput = L.tput ? p.tput : nullptr;
    ps.cut_depth = L.cut_depth;
    ps.depth_pair[0] = ps.max_depth;  // (the two once more, for the TYP instantiations' one load: split_depths)
    ps.depth_pair[1] = L.cut_depth;
    const int args = (p.stats != nullptr ? 1 : 0) | L.tris << 1 | L.typ << 2 | L.max32 << 3 | (L.hq_cap > 0 ? 1 : 0) << 4 | L.lds_scene << 5 | L.axis << 6;
    return with_const<256>(args, [&](auto c) {
        constexpr int I = decltype(c)::value, AXIS = I >> 6;
        constexpr bool STATS = I & 1, TRIS = I & 2, TYP = I & 4, MAX32 = I & 8, HQ = I & 16, LDS_SCENE = I & 32;
        constexpr auto here = [](int kernel) { return kernel_exists(kThisCopy, kPassRender, kernel, TRIS, TYP, MAX32, HQ, AXIS, LDS_SCENE); };
        if constexpr (here(0))
            if (L.kernel == 0) render_static_kernel<STATS, TRIS><<<g, b, lds, stream>>>(p);
        if constexpr (here(1))
            if (L.kernel == 1) render_refill_kernel<STATS, TRIS><<<g, b, lds, stream>>>(p);
#if FLUX_FAST  // (the STRICT copy does not declare these)
        if constexpr (here(2))
            if (L.kernel == 2) render_split_kernel<STATS, MAX32, TYP, HQ, AXIS><<<g, b, lds, stream>>>(ps, L.hq_cap, L.hq_th, L.hq_bits, L.uniform_a);
        if constexpr (here(3))
            if (L.kernel == 3) render_bvh_kernel<STATS><<<g, b, lds, stream>>>(p);
        if constexpr (here(4))
            if (L.kernel == 4) render_bvh4_kernel<STATS, LDS_SCENE, TYP><<<g, b, lds, stream>>>(p);
#endif
        return hipGetLastError();
    });
}

