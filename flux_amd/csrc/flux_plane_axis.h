// flux_plane_axis.h -- the split kernel's first scan plane when its stored normal is an axis (render_body.inc scan_shapes_primary,
// scan_shapes_fast<.., TYP, ZF = 0>).  One source for the host's classification (scene_build.cpp), the kernel's reduced expressions and
// the CPU test that compares them with the general ones in every fusion a compiler may pick (tests/plane_axis_selftest.cpp).
//
// The general test (Plane::hit, shapes.rs:135-152) forms num = (p - o).n, den = d.n and t = num / den.  With n = s e_a (s = +1 or -1,
// the other two components +0 or -0) every product but one multiplies by an exact zero or an exact one:
//     num = s (p_a - o_a) + z1 + z2,    den = s d_a + z3 + z4,
// where each z is (p_b - o_b) 0 or d_b 0: a zero of either sign while that factor is finite, NaN when it is infinite or NaN.  Adding a
// zero to a NON-ZERO value changes nothing, fused or not, in any order; so with every z a zero and d_a != 0, den = s d_a exactly, and
// num = s (p_a - o_a) exactly unless p_a - o_a is itself zero.  IEEE division takes the sign of the quotient from the signs of its
// operands and its magnitude from their magnitudes: s cancels, and
//     t = (p_a - o_a) / d_a
// bit for bit.  Where p_a - o_a is zero, num is a zero whose sign depends on s, on the signs of the z's and on the fusion; t is then a
// zero of either sign -- den is not zero -- and fails t > T_MIN whichever it is: the plane is missed in both forms, and the scans read
// the distance only beside a hit.
//
// What the reduced form needs, then (plane_axis_admits): d_a != 0 (a zero d_a makes den a zero of a sign that depends on the other
// components and on the fusion: t = +-inf, and +inf is a hit); the other two components of d finite; the other two components of o such
// that p_b - o_b is finite.  The classification keeps the plane's own point below 1e300 in every component, so |o_b| < 1e300 will do.
// The predicate asks the same of o_a and d_a -- a NaN there makes both forms NaN, of payloads no test should hang on -- and the kernel's
// votes imply it (render_body.inc): a wave with a lane outside it runs the general code.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FLUX_PA_HD __host__ __device__ inline
#else
#define FLUX_PA_HD inline
#endif

namespace flux {

constexpr int kPlaneAxisNone = 0, kPlaneAxisX = 1, kPlaneAxisY = 2, kPlaneAxisZ = 3;
constexpr double kPlaneAxisRange = 1e300;  // the plane's point, and the origins the predicate admits, stay below it

// (host) The axis of a plane's STORED normal (never normalised, as the scan uses it) and point: one component equal to +1 or -1, the
// other two comparing equal to zero (either sign), every component of the point below kPlaneAxisRange.  A NaN fails every compare.
inline int plane_axis_of(double nx, double ny, double nz, double px, double py, double pz) {
    if (!(std::fabs(px) < kPlaneAxisRange && std::fabs(py) < kPlaneAxisRange && std::fabs(pz) < kPlaneAxisRange)) return kPlaneAxisNone;
    if (std::fabs(nx) == 1.0 && ny == 0.0 && nz == 0.0) return kPlaneAxisX;
    if (nx == 0.0 && std::fabs(ny) == 1.0 && nz == 0.0) return kPlaneAxisY;
    if (nx == 0.0 && ny == 0.0 && std::fabs(nz) == 1.0) return kPlaneAxisZ;
    return kPlaneAxisNone;
}

// (host) The camera's side, for the split kernel's primary rays (render_body.inc primary_ray_px): every scalar finite and below 1e60.
// The sample tables hold points of the unit square and the unit disc, so every product the ray generation forms has at most four such
// factors (aps (col - half_w) factor U: below 1e240) and every sum a few such terms: the origin and the unnormalised direction v are
// finite, the origin far below kPlaneAxisRange.  The direction is v inv with ONE inv = frsqrt(v.v) for the three components: finite
// (v.v positive and finite: |v_i inv| <= 1 to rounding), or NaN in all three (v.v zero or overflowed: frsqrt's first product is
// 0 inf).  So a primary ray's d_a that is neither zero nor NaN has finite companions.
inline bool plane_axis_camera_ok(const double *scalars, int n) {
    for (int k = 0; k < n; k++)
        if (!(std::fabs(scalars[k]) < 1e60)) return false;
    return true;
}

// The predicate, per lane: what the reduced form needs (above).  Negated compares: a NaN anywhere refuses.
FLUX_PA_HD bool plane_axis_admits(int axis, double ox, double oy, double oz, double dx, double dy, double dz) {
    const double da = axis == kPlaneAxisX ? dx : axis == kPlaneAxisY ? dy : dz;
    if (axis == kPlaneAxisNone || !(__builtin_fabs(da) > 0.0)) return false;
    if (!(__builtin_fabs(dx) < __builtin_inf() && __builtin_fabs(dy) < __builtin_inf() && __builtin_fabs(dz) < __builtin_inf())) return false;
    return __builtin_fabs(ox) < kPlaneAxisRange && __builtin_fabs(oy) < kPlaneAxisRange && __builtin_fabs(oz) < kPlaneAxisRange;
}

// What BOTH of the kernel's votes ask of den = d_a, in place of the predicate's d_a != 0: the f32 image of d_a is a normal number.  One
// class test (its mask in a scalar register) of a value phase B's filter converts anyway.  A NaN, an infinity, a zero and every |d_a| below
// 2^-126 (1 - 2^-25) or beyond f32 are refused: such a wave runs the general code with `/`.  It is what lets the reduced arms divide
// without the general division's scaffolding (plane_div_unscaled, below).
FLUX_PA_HD bool plane_div_admits(double da) { return __builtin_isnormal((float)da); }
// (host) ... and of the plane: the axis component of its point below kPlaneDivPoint
constexpr double kPlaneDivPoint = 1e150;
inline bool plane_div_point_ok(double pa) { return std::fabs(pa) < kPlaneDivPoint; }

// Phase B's vote as the kernel takes it, per lane, from the ray in f32 (render_body.inc: o.o and o.u as the sphere filter forms them):
//   |o|^2 < 0.999e6 in f32   every component of o is finite and below 1e3 (an infinite or NaN component makes the sum infinite or NaN,
//                            a component beyond f32 converts to infinity);
//   |o.u| finite in f32      every component of d is finite: an infinite or NaN d_i (or one beyond f32) converts to infinity or NaN, its
//                            product with a finite o_i is infinite or -- o_i = 0 -- NaN, and a sum of fused multiply-adds that takes
//                            in an infinity or a NaN stays one or the other;
//   d_z != 0                 the pass's own rule for direction.z;
//   plane_div_admits(d_a)    the axis component: not zero, and of a size the unscaled division takes (below).
FLUX_PA_HD bool plane_axis_admits_b(int axis, double ox, double oy, double oz, double dx, double dy, double dz) {
    const float ofx = (float)ox, ofy = (float)oy, ofz = (float)oz;
    const float oo = __builtin_fmaf(ofz, ofz, __builtin_fmaf(ofy, ofy, ofx * ofx));
    const float ou = __builtin_fmaf(ofz, (float)dz, __builtin_fmaf(ofy, (float)dy, ofx * (float)dx));
    const double da = axis == kPlaneAxisX ? dx : axis == kPlaneAxisY ? dy : dz;
    return axis != kPlaneAxisNone && !(dz == 0.0) && oo < 0.999e6f && __builtin_fabsf(ou) < 3.0e38f && plane_div_admits(da);
}

// ---- The reduced arms' division t = num / den without the scaffolding of the general one.
// The compiler's f64 division on this target is: den' = div_scale(den), num' = div_scale(num) (each operand times 2^+-128 where the
// reciprocal, the quotient or the residual would leave the normal range; the operand itself otherwise), r = rcp(den'), two Newton steps
// r += r (1 - den' r), q = num' r, the residual e = num' - den' q, t = e r + q (scaled back where an operand was), and a fix-up that
// replaces t for zero, infinite and NaN operands.  Where neither operand is scaled and both are finite and non-zero the scaffolding is
// idle -- both scale instructions return their operand, the last step is a plain fused multiply-add, the fix-up returns t -- and
// plane_div_unscaled below, the same operations on the same operands in the same order, has the bits of num / den.
//
// When is it idle?  The scale instruction's rules, with e(x) the unbiased exponent of x: an operand is scaled when
//     den is denormal;   1 / den is denormal (e(den) >= 1022);   e(num) - e(den) >= 768;   num / den is denormal
//     (e(num) - e(den) <= -1023);   num is tiny (e(num) <= 53 - 1023);   (and either operand zero: the fix-up's case.)
// The votes bound den (plane_div_admits): its f32 image is a NORMAL number, so -127 <= e(den) <= 127 (the smallest den admitted
// rounds up to 2^-126), den is finite, not zero, not NaN.  The reduced num is p_a - o_a with |p_a| < kPlaneDivPoint = 1e150 on the
// host's word (scene_build.cpp sets the axis only for such a plane) and |o_a| < 1e3 in phase B (its vote) or, in phase A, the lens
// point of a camera inside plane_axis_camera_ok: e + lens (U, V) of scalars below 1e60, below 2^401.  So |num| < 2^499 -- in a scene of
// ordinary size, below 2e3.  For 2^-894 <= |num| < 2^499 no rule applies: e(num) - e(den) lies in [-1021, 625], 1 / den in
// [2^-128, 2^128], and the residual, a multiple of 2^(e(num) - 105), is a normal number or zero: bit for bit num / den.
// (tests/plane_div_selftest.cpp restates the rules and holds the function to `/` over these operands.)
//
// A num below 2^-894 in magnitude -- zeros and denormals among them -- needs no guard.  Every operation of the function is then
// finite (|r| <= 2^128, |q| <= 2^-765) and so is its result, of magnitude below 2^-764; num / den is as small.  The two may differ
// in their last bits, or in the sign of a zero (num = -0: the residual's sum yields +0); both fail t > T_MIN = 5e-4, the only question
// either scan asks of the first plane's t, and `tb` is read only beside best >= 0.  A path meets such a num when its origin lies ON
// the plane to within 2^-894: the plane is missed in both forms.

// t = num / den by the compiler's sequence without the two scale instructions and the fix-up; `seed` approximates 1 / den (the device's
// v_rcp_f64; the CPU test's perturbed reciprocal).  Explicit fused multiply-adds and one product: nothing here may be contracted,
// re-associated or recognised as a division under the build's flags (-fno-fast-math; fp contract only ever fuses a product INTO a sum).
FLUX_PA_HD double plane_div_unscaled(double num, double den, double seed) {
    double r = seed;
    r = __builtin_fma(r, __builtin_fma(-den, r, 1.0), r);
    r = __builtin_fma(r, __builtin_fma(-den, r, 1.0), r);
    const double q = num * r;
    const double e = __builtin_fma(-den, q, num);
    return __builtin_fma(e, r, q);
}
#if defined(__HIPCC__)
__device__ __forceinline__ double plane_div_unscaled(double num, double den) { return plane_div_unscaled(num, den, __builtin_amdgcn_rcp(den)); }
#endif

// The reduced expressions.  `axis` is a template argument in the kernel (render_split_kernel<.., AXIS>): the branches fold away.
FLUX_PA_HD void plane_axis_num_den(int axis, double px, double py, double pz, double ox, double oy, double oz, double dx, double dy,
                                   double dz, double &num, double &den) {
    if (axis == kPlaneAxisY) {
        num = py - oy;
        den = dy;
    } else if (axis == kPlaneAxisX) {
        num = px - ox;
        den = dx;
    } else {
        num = pz - oz;
        den = dz;
    }
}

}  // namespace flux
