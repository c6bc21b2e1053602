// flux_env_verdict.h -- the split kernel's environment shortcut decided in f32 (render_body.inc scan_shapes_fast<ENV_SHORT>).
// One source for the kernel and for the CPU test that compares it with the exact predicate (tests/env_verdict_selftest.cpp):
// plain C++, every fused multiply-add spelled out, nothing left to contraction.
//
// The question.  A secondary ray o + t u (|u| = 1) starts inside the scene's Emissive `invert` sphere (centre p, radius r) and has a
// best hit so far at distance tb (or none).  The sphere's far root t_env is nearer than tb exactly when the best hit POINT lies
// outside the sphere: with hb = (o - p).u and c = |o - p|^2 - r^2,
//     g = c + tb (tb + 2 hb) = |o + tb u - p|^2 - r^2,
// and for an origin inside (c < 0, tb > 0) the quadratic t^2 + 2 hb t + c has one positive root, t_env, so t_env < tb <=> g > 0.
// The f64 shortcut decides the same thing as "s = tb + hb > 0 and hb^2 - c < s^2"; hb^2 - c - s^2 = -g, and g > 0 implies s > 0
// (s <= 0 means hb <= -tb, so tb (tb + 2 hb) <= -tb^2 and g <= c - tb^2 < 0).
//
// The error bound.  Every operand is rounded to f32 once (relative 2^-24 = 6e-8) and c, hb, g are chains of f32 fused multiply-adds.
// With M = o.o + p.p + r^2 every intermediate of c is at most (|o| + |p|)^2 + r^2 <= 2 M, so its roundings -- six conversions (each
// enters a product of two magnitudes), three operations of o.o, three of the chain, the constant's own and the last addition --
// sum to less than 30 x 6e-8 x M = 1.8e-6 M.  g adds tb^2 and 2 tb hb: tb's conversion and the two operations give 4 x 6e-8 tb^2,
// and hb's error (seven roundings of magnitudes below |o| + |p|) times 2 tb is at most 7 x 6e-8 (tb^2 + (|o| + |p|)^2) <=
// 4.2e-7 (tb^2 + 2 M).  In all |g32 - g| < 2.7e-6 (M + tb^2) and |c32 - c| < 1.8e-6 M: the margin is the filter's 8e-6 of the same
// squared magnitudes (flux_device.h DevScanSphere32), three times the bound.  The f64 shortcut calls a lane "too close to call"
// within env_eps (dq + s^2) <= 1e-9 x 8 (M + tb^2) of g = 0 and "deep" for c < env_deep: a lane decided here with the margin is
// decided there, to the same answer -- so a wave whose lanes are all decided here gets from the f64 shortcut what it gets here.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FLUX_ENV_HD __host__ __device__ inline
#else
#define FLUX_ENV_HD inline
#endif

namespace flux {

constexpr int kEnvUndecided = 0, kEnvWins = 1, kEnvLoses = 2;
constexpr float kEnvMargin32 = 8e-6f;

// The environment's side, rounded once on the host (scene_build.cpp): MINUS the centre, p.p - r^2, p.p + r^2 and env_deep.
struct EnvSphere32 {
    float npx, npy, npz;
    float ppr;   // p.p - r^2
    float mag;   // p.p + r^2: the sphere's share of the margin's magnitudes
    float deep;  // RenderParams::env_deep: an origin counts as inside below it
};

// (host) px, py, pz, rr: the sphere's f64 scan record; deep: RenderParams::env_deep, rounded DOWN so that "below it in f32" is never
// less than "below it".  The centre negated, as the filter's records hold it (flux_device.h DevScanSphere32).
inline EnvSphere32 env_sphere32(double px, double py, double pz, double rr, double deep) {
    const double pp = px * px + py * py + pz * pz;
    float d = (float)deep;
    if ((double)d > deep) d = std::nextafterf(d, -INFINITY);
    return EnvSphere32{-(float)px, -(float)py, -(float)pz, (float)(pp - rr), (float)(pp + rr), d};
}

// The ray's side, formed before the scan's candidate loop: three values cross it.
struct EnvRay32 {
    float hb2;  // 2 hb
    float cm;   // c - m: what "the hit point is outside" is decided from
    float cp;   // c + m: what "the origin is inside" and "the hit point is inside" are decided from
};

// o2 = 2 o and u: the ray in f32; ou = o.u and oo = o.o as the sphere filter forms them (render_body.inc filter_ray32_f).
FLUX_ENV_HD EnvRay32 env_ray32(const EnvSphere32 &E, float o2x, float o2y, float o2z, float ux, float uy, float uz, float ou, float oo) {
    const float hb = __builtin_fmaf(E.npx, ux, __builtin_fmaf(E.npy, uy, __builtin_fmaf(E.npz, uz, ou)));
    const float c = __builtin_fmaf(E.npx, o2x, __builtin_fmaf(E.npy, o2y, __builtin_fmaf(E.npz, o2z, oo))) + E.ppr;
    const float m = kEnvMargin32 * (oo + E.mag);
    return EnvRay32{2.0f * hb, c - m, c + m};
}

// g with the margin taken off and put on: g_lo <= g - m, g_hi >= g + m.  tb: the best hit's distance so far in f32.  tb's share of
// the margin, 8e-6 tb^2, is folded into the coefficient of tb^2, so that an infinite tb -- a plane parallel to the ray, or a distance
// beyond f32 -- gives +inf, not inf - inf: the environment wins, as it does in f64.
FLUX_ENV_HD void env_g32(const EnvRay32 &R, float tb, float &g_lo, float &g_hi) {
    g_lo = __builtin_fmaf(tb, __builtin_fmaf(1.0f - kEnvMargin32, tb, R.hb2), R.cm);
    g_hi = __builtin_fmaf(tb, __builtin_fmaf(1.0f + kEnvMargin32, tb, R.hb2), R.cp);
}

// The verdict of one lane (has_best false: tb means nothing).  Every test is one that a NaN fails: a NaN anywhere leaves the lane
// undecided.  The kernel takes the same three compares as lane masks and votes on them (scan_shapes_fast).
FLUX_ENV_HD int env_verdict32(const EnvSphere32 &E, const EnvRay32 &R, float tb, bool has_best) {
    if (!(R.cp < E.deep)) return kEnvUndecided;
    if (!has_best) return kEnvWins;
    float g_lo, g_hi;
    env_g32(R, tb, g_lo, g_hi);
    if (g_lo > 0.0f) return kEnvWins;
    if (g_hi < 0.0f) return kEnvLoses;
    return kEnvUndecided;
}

}  // namespace flux
