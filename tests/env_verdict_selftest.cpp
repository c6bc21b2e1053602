// The split kernel's f32 environment verdict (flux_amd/csrc/flux_env_verdict.h) against the exact predicate, CPU only
// (tests/test_env_verdict.py builds and runs it; the header is the kernel's own source).
//   usage: env_verdict_selftest
// Exact: c = |o - p|^2 - r^2 and g = c + tb (tb + 2 hb) in long double from the f64 inputs.  Three conditions:
//   1. never a wrong "wins" (needs c < env_deep and, beside a best hit, g > 0) or "loses" (c < env_deep, a best hit, g < 0);
//   2. with demo2's environment (r = 100, centre 0) every case is decided whose origin is within 0.9 r of the centre and whose hit
//      point is inside 0.99 r or outside 1.01 r: the fallback to the f64 shortcut cannot be the common case;
//   3. a decided lane is one the f64 shortcut (render_body.inc scan_shapes_fast) decides too -- deep, not "too close to call" --
//      and to the same answer, so a wave the verdict serves gets what the shortcut would have given it.
// Prints one "ok <name>" per family and "all ok" at the end; exits 1 on the first failure.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>

#include "../flux_amd/csrc/flux_env_verdict.h"

using namespace flux;

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint64_t next_u64() {  // splitmix64
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static double uni() { return (double)(next_u64() >> 11) * (1.0 / 9007199254740992.0); }  // [0, 1)
static double sym() { return 2.0 * uni() - 1.0; }
static void unit(double &x, double &y, double &z) {
    double n;
    do {
        x = sym(); y = sym(); z = sym();
        n = x * x + y * y + z * z;
    } while (n < 1e-3 || n > 1.0);
    n = 1.0 / std::sqrt(n);
    x *= n; y *= n; z *= n;
}

struct Sphere {
    double px, py, pz, r;
};
struct Counts {
    long cases = 0, wins = 0, loses = 0, undecided = 0;
};
static const double kTMin = 0.0005, kEnvEps = 1e-9;

// one case; `must_decide`: condition 2 applies.  Returns false (after printing) on a violated condition.
static bool check(const Sphere &S, double ox, double oy, double oz, double ux, double uy, double uz, double tb, bool has_best, bool must_decide,
                  Counts &n) {
    const double rr = S.r * S.r;
    const double env_radius = S.r * (1.0 + 1e-12), env_deep = -(4.0 * kTMin) * env_radius;  // scene_build.cpp
    const EnvSphere32 E = env_sphere32(S.px, S.py, S.pz, rr, env_deep);
    // the ray's side as filter_ray32_f forms it
    const float ofx = (float)ox, ofy = (float)oy, ofz = (float)oz, ufx = (float)ux, ufy = (float)uy, ufz = (float)uz;
    const float ouf = __builtin_fmaf(ofz, ufz, __builtin_fmaf(ofy, ufy, ofx * ufx));
    const float oof = __builtin_fmaf(ofz, ofz, __builtin_fmaf(ofy, ofy, ofx * ofx));
    const EnvRay32 R = env_ray32(E, 2.0f * ofx, 2.0f * ofy, 2.0f * ofz, ufx, ufy, ufz, ouf, oof);
    const int v = env_verdict32(E, R, (float)tb, has_best);
    n.cases++;
    (v == kEnvWins ? n.wins : v == kEnvLoses ? n.loses : n.undecided)++;
    // exact
    const long double tx = (long double)ox - S.px, ty = (long double)oy - S.py, tz = (long double)oz - S.pz;
    const long double hb = tx * ux + ty * uy + tz * uz;
    const long double c = tx * tx + ty * ty + tz * tz - (long double)rr;
    const long double g = c + (long double)tb * ((long double)tb + 2.0L * hb);
    bool ok = true;
    if (v != kEnvUndecided && !(c < (long double)env_deep)) ok = false;
    if (v == kEnvWins && has_best && !(g > 0.0L)) ok = false;
    if (v == kEnvLoses && !(has_best && g < 0.0L)) ok = false;
    if (must_decide && v == kEnvUndecided) ok = false;
    // the f64 shortcut's own decision (finite squares only: beyond them it calls the lane close and leaves it to the exact roots)
    if (ok && v != kEnvUndecided && std::fabs(tb) < 1e150) {
        const double dx = ox - S.px, dy = oy - S.py, dz = oz - S.pz;
        const double hb64 = __builtin_fma(dz, uz, __builtin_fma(dy, uy, dx * ux));
        const double c64 = __builtin_fma(dx, dx, __builtin_fma(dy, dy, __builtin_fma(dz, dz, -rr)));
        const double dq = __builtin_fma(hb64, hb64, -c64);
        const double s = tb + hb64, s2 = s * s;
        const bool deep = c64 < env_deep, close = std::fabs(dq - s2) <= kEnvEps * (dq + s2);
        if (!deep || (has_best && close)) ok = false;
        if ((v == kEnvWins) != (!has_best || (s > 0.0 && dq < s2))) ok = false;
    }
    if (!ok)
        std::printf("FAILED verdict %d best %d must_decide %d: p (%a %a %a) r %a o (%a %a %a) u (%a %a %a) tb %a  c %Lg g %Lg\n", v, (int)has_best,
                    (int)must_decide, S.px, S.py, S.pz, S.r, ox, oy, oz, ux, uy, uz, tb, c, g);
    return ok;
}

// radius log-uniform in [0.5, 1e3]; the centre at the origin or up to `off` away on each axis
static Sphere random_sphere(double off) {
    const double r = 0.5 * std::pow(2000.0, uni());
    return Sphere{off * sym(), off * sym(), off * sym(), r};
}

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const long kN = 1000000;
    Counts n;
    // 1. uniformly random rays and hit distances, origins anywhere within 1.2 r of a centre up to 900 off the origin
    for (long k = 0; k < kN; k++) {
        const Sphere S = random_sphere(k & 1 ? 900.0 : 0.0);
        double dx, dy, dz, ux, uy, uz;
        unit(dx, dy, dz);
        unit(ux, uy, uz);
        const double a = 1.2 * S.r * std::cbrt(uni());
        const double tb = 3.0 * S.r * uni() * uni();
        if (!check(S, S.px + a * dx, S.py + a * dy, S.pz + a * dz, ux, uy, uz, tb, (k & 7) != 0, false, n)) return 1;
    }
    std::printf("ok random rays: %ld cases, %ld wins, %ld loses, %ld undecided\n", n.cases, n.wins, n.loses, n.undecided);
    // 2. origins and hit points within +-10 margins of the sphere: the hit point is placed at radius r (1 + k m), m the margin's
    //    relative size, and the origin likewise in every other case
    n = Counts();
    for (long k = 0; k < kN; k++) {
        const Sphere S = random_sphere(k & 1 ? 300.0 : 0.0);
        double dx, dy, dz, hx, hy, hz;
        unit(dx, dy, dz);
        unit(hx, hy, hz);
        const double m = 8e-6 * 3.0;  // the margin over r^2, roughly, for a centre near the origin
        const double ro = (k & 2) ? S.r * (1.0 + 10.0 * m * sym()) : S.r * 0.95 * std::cbrt(uni());
        const double rh = S.r * (1.0 + 10.0 * m * sym());
        const double ox = S.px + ro * dx, oy = S.py + ro * dy, oz = S.pz + ro * dz;
        double ux = S.px + rh * hx - ox, uy = S.py + rh * hy - oy, uz = S.pz + rh * hz - oz;
        const double tb = std::sqrt(ux * ux + uy * uy + uz * uz);
        if (!(tb > 0.0)) continue;
        ux /= tb; uy /= tb; uz /= tb;
        if (!check(S, ox, oy, oz, ux, uy, uz, tb, true, false, n)) return 1;
    }
    std::printf("ok around the margins: %ld cases, %ld wins, %ld loses, %ld undecided\n", n.cases, n.wins, n.loses, n.undecided);
    // 3. tb of 0, denormal, +inf, NaN, huge, and no best hit at all
    n = Counts();
    const double special[] = {0.0, 4.9e-324, 1e-310, inf, nan, 1e30, 1e39, 1e200, kTMin};
    for (long k = 0; k < kN / 4; k++) {
        const Sphere S = random_sphere(k & 1 ? 900.0 : 0.0);
        double dx, dy, dz, ux, uy, uz;
        unit(dx, dy, dz);
        unit(ux, uy, uz);
        const double a = 1.1 * S.r * uni();
        for (const double tb : special)
            if (!check(S, S.px + a * dx, S.py + a * dy, S.pz + a * dz, ux, uy, uz, tb, true, false, n)) return 1;
        if (!check(S, S.px + a * dx, S.py + a * dy, S.pz + a * dz, ux, uy, uz, nan, false, false, n)) return 1;
    }
    {   // NaN stays undecided, an infinite distance wins
        const Sphere S{0.0, 0.0, 0.0, 100.0};
        Counts one;
        if (!check(S, 1.0, 2.0, 3.0, 0.0, 1.0, 0.0, nan, true, false, one) || one.undecided != 1) return std::printf("FAILED NaN tb\n"), 1;
        if (!check(S, 1.0, 2.0, 3.0, 0.0, 1.0, 0.0, inf, true, false, one) || one.wins != 1) return std::printf("FAILED infinite tb\n"), 1;
        if (!check(S, nan, 2.0, 3.0, 0.0, 1.0, 0.0, 5.0, true, false, one) || one.undecided != 2) return std::printf("FAILED NaN origin\n"), 1;
        if (!check(S, 1.0, 2.0, 3.0, 0.0, 1.0, 0.0, 0.0, true, false, one) || one.loses != 1) return std::printf("FAILED zero tb\n"), 1;
    }
    std::printf("ok special distances: %ld cases, %ld wins, %ld loses, %ld undecided\n", n.cases, n.wins, n.loses, n.undecided);
    // 4. the cap, demo2's environment: origin within 0.9 r, hit point inside 0.99 r or outside 1.01 r (out to 1e4 r) -- all decided
    n = Counts();
    const Sphere D{0.0, 0.0, 0.0, 100.0};
    for (long k = 0; k < kN; k++) {
        double dx, dy, dz, hx, hy, hz;
        unit(dx, dy, dz);
        unit(hx, hy, hz);
        const double ro = 0.9 * D.r * std::cbrt(uni());
        const double rh = (k & 1) ? 0.99 * D.r * std::cbrt(uni()) : 1.01 * D.r * std::pow(1e4, uni() * uni());
        const double ox = ro * dx, oy = ro * dy, oz = ro * dz;
        double ux = rh * hx - ox, uy = rh * hy - oy, uz = rh * hz - oz;
        const double tb = std::sqrt(ux * ux + uy * uy + uz * uz);
        if (!(tb > 1e-6)) continue;
        ux /= tb; uy /= tb; uz /= tb;
        if (!check(D, ox, oy, oz, ux, uy, uz, tb, true, true, n)) return 1;
        if ((k & 15) == 0 && !check(D, ox, oy, oz, ux, uy, uz, tb, false, true, n)) return 1;
    }
    if (n.undecided != 0) return std::printf("FAILED cap: %ld undecided\n", n.undecided), 1;
    std::printf("ok cap: %ld cases, %ld wins, %ld loses, %ld undecided\n", n.cases, n.wins, n.loses, n.undecided);
    std::printf("all ok\n");
    return 0;
}
