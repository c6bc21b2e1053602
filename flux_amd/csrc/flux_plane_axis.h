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

// Phase B's vote as the kernel takes it, per lane, from the ray in f32 (render_body.inc: o.o and o.u as the sphere filter forms them):
//   |o|^2 < 0.999e6 in f32   every component of o is finite and below 1e3 (an infinite or NaN component makes the sum infinite or NaN,
//                            a component beyond f32 converts to infinity);
//   |o.u| finite in f32      every component of d is finite: an infinite or NaN d_i (or one beyond f32) converts to infinity or NaN, its
//                            product with a finite o_i is infinite or -- o_i = 0 -- NaN, and a sum of fused multiply-adds that takes
//                            in an infinity or a NaN stays one or the other;
//   d_a != 0, d_z != 0       the axis component, and the pass's own rule for direction.z.
FLUX_PA_HD bool plane_axis_admits_b(int axis, double ox, double oy, double oz, double dx, double dy, double dz) {
    const float ofx = (float)ox, ofy = (float)oy, ofz = (float)oz;
    const float oo = __builtin_fmaf(ofz, ofz, __builtin_fmaf(ofy, ofy, ofx * ofx));
    const float ou = __builtin_fmaf(ofz, (float)dz, __builtin_fmaf(ofy, (float)dy, ofx * (float)dx));
    const double da = axis == kPlaneAxisX ? dx : axis == kPlaneAxisY ? dy : dz;
    return axis != kPlaneAxisNone && !(dz == 0.0) && oo < 0.999e6f && __builtin_fabsf(ou) < 3.0e38f && !(da == 0.0);
}

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
