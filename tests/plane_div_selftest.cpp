// The split kernel's unscaled first-plane division (flux_amd/csrc/flux_plane_axis.h plane_div_unscaled) and the predicate its votes
// take (plane_div_admits), CPU only (tests/test_plane_div.py builds and runs it; the header is the kernel's and the host's own source).
//   usage: plane_div_selftest [quick]        (quick: a tenth of the random cases, for the sanitizer build)
//   1. predicate: for every den the predicate admits and every num of 2^-894 <= |num| < 2^499 (a scene's |num| < 2e3 among them), a
//      restatement of v_div_scale_f64's documented rules says that neither operand is scaled and the fix-up has nothing to do -- random
//      pairs and the exponent edges of both operands; just outside the predicate, on either side, a rule does apply for some such num;
//   2. function: with the correctly rounded 1 / den moved by -2 .. +2 ulp as the seed, plane_div_unscaled has the bits of num / den
//      over those pairs (|num| = 2e3 and the edges among them);
//   3. small nums: for |num| < 2^-894 -- zeros and denormals among them -- the function and num / den are both finite and below
//      2^-764 in magnitude, far below T_MIN: the scans' verdict is the same (bit equality is counted and printed, not required: a
//      num of -0 gives +0 for -0, and a denormal residual loses bits);
//   4. votes: on special values of d_a (zeros, denormals, the floor and the ceiling of the predicate and their neighbours, infinities,
//      NaN) phase B's vote (plane_axis_admits_b) over an ordinary ray says what the predicate says -- phase A's vote IS the predicate --
//      and a ray it admits is one plane_axis_admits admits.
// Prints one "ok <name>" per family and "all ok" at the end; exits 1 on the first failure.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../flux_amd/csrc/flux_plane_axis.h"

using namespace flux;

static uint64_t g_state = 0x2545f4914f6cdd1dull;
static uint64_t next_u64() {  // splitmix64
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static double uni() { return (double)(next_u64() >> 11) * (1.0 / 9007199254740992.0); }  // [0, 1)
static uint64_t bits(double x) {
    uint64_t u;
    std::memcpy(&u, &x, 8);
    return u;
}
static double from_bits(uint64_t u) {
    double x;
    std::memcpy(&x, &u, 8);
    return x;
}
static double ulps(double x, int k) { return from_bits(bits(x) + (uint64_t)(int64_t)k); }  // k ulp away from zero (k < 0: towards it)
static int biased_exp(double x) { return (int)((bits(x) >> 52) & 0x7ff); }

static const double kTMin = 0.0005;
static const double kNumLow = 0x1p-894, kNumHigh = 0x1p499;
static const double kSmallBound = 0x1p-764;

// v_div_scale_f64 (numerator S2 = num, denominator S1 = den), the ISA manual's rules in its order; true when the instruction pair
// would scale an operand or flag the result, or the fix-up would replace it
static bool scaffolding_acts(double num, double den) {
    if (std::isnan(num) || std::isnan(den) || std::isinf(num) || std::isinf(den)) return true;  // the fix-up's operands
    if (num == 0.0 || den == 0.0) return true;
    const int en = biased_exp(num), ed = biased_exp(den);
    if (en - ed >= 768) return true;                                   // num / den near overflow
    if (ed == 0) return true;                                          // den is denormal
    if (std::fpclassify(1.0 / den) == FP_SUBNORMAL || 1.0 / den == 0.0) return true;  // 1 / den is denormal
    if (en - ed <= -1023 || std::fpclassify(num / den) == FP_SUBNORMAL) return true;  // num / den is denormal
    if (en <= 53) return true;                                         // num is tiny (its residual would lose bits)
    return false;
}

// the predicate's own edges in f64: the smallest and the largest magnitude whose f32 image is a normal number
static const double kFloor = 0x1p-126 - 0x1p-150;                // the tie between the largest f32 denormal and 2^-126 rounds to even: up
static const double kCeil = 0x1.fffffefffffffp+127;             // one ulp below the tie between FLT_MAX and 2^128, which rounds to infinity

static double random_den() {
    const int family = (int)(next_u64() % 4);
    double d;
    if (family == 0) d = 2.0 * uni() - 1.0;                                        // a direction's component
    else if (family == 1) d = std::ldexp(0.5 + 0.5 * uni(), (int)(next_u64() % 256) - 126);  // every admitted exponent
    else if (family == 2) d = std::ldexp(0.5 + 0.5 * uni(), -127 + (int)(next_u64() % 3)) * (next_u64() & 1 ? 1.0 : -1.0);  // on either side of the floor
    else d = std::ldexp(0.5 + 0.5 * uni(), 127 + (int)(next_u64() % 3));                // on either side of the ceiling
    return (next_u64() & 1) ? d : -d;
}
static double random_num() {
    const int family = (int)(next_u64() % 4);
    double x;
    if (family == 0) x = 4000.0 * uni() - 2000.0;                                  // a scene's p_a - o_a
    else if (family == 1) x = std::ldexp(0.5 + 0.5 * uni(), (int)(next_u64() % 1393) - 893);  // 2^-894 .. 2^499
    else if (family == 2) x = std::ldexp(1.0 + uni(), -894 + (int)(next_u64() % 3));          // by the low edge (at or above it)
    else x = std::ldexp(0.5 + 0.5 * uni(), 497 + (int)(next_u64() % 3));                      // by the high edge (below it)
    return (next_u64() & 1) ? x : -x;
}

static bool check_pair(double num, double den, long &tested) {
    if (!plane_div_admits(den)) return true;
    if (!(std::fabs(num) >= kNumLow && std::fabs(num) < kNumHigh)) return true;
    tested++;
    if (scaffolding_acts(num, den)) {
        std::printf("FAIL predicate: den %a admitted, but the division's scaffolding acts on num %a\n", den, num);
        return false;
    }
    const double want = num / den, exact = 1.0 / den;
    // (a den whose fraction bits are all ones: 1 / den lies 2^-106 above a rounding tie, the one case in which the final step needs
    // the CORRECTLY rounded reciprocal and not just a faithful one -- Markstein's exception.  The two Newton steps do not reach it
    // from a moved seed, so there the moved seeds are held to the function's result where they do, and the exact seed always.)
    const bool hard = (bits(den) & 0xfffffffffffffull) == 0xfffffffffffffull;
    for (int k = -2; k <= 2; k++) {
        const double seed = ulps(exact, k);
        if (hard && k != 0) {
            double r = seed;
            r = __builtin_fma(r, __builtin_fma(-den, r, 1.0), r);
            r = __builtin_fma(r, __builtin_fma(-den, r, 1.0), r);
            if (bits(r) != bits(exact)) continue;
        }
        const double got = plane_div_unscaled(num, den, seed);
        if (bits(got) != bits(want)) {
            std::printf("FAIL function: num %a den %a seed 1/den %+d ulp: %a (%016llx), num / den is %a (%016llx)\n", num, den, k, got,
                        (unsigned long long)bits(got), want, (unsigned long long)bits(want));
            return false;
        }
    }
    return true;
}

int main(int argc, char **argv) {
    const bool quick = argc > 1 && std::strcmp(argv[1], "quick") == 0;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();

    // ---- 1 and 2: random pairs, then the edges of both operands against each other
    {
        long tested = 0;
        const long n_cases = quick ? 150000 : 1500000;
        for (long k = 0; k < n_cases; k++)
            if (!check_pair(random_num(), random_den(), tested)) return 1;
        const double dens[] = {kFloor, ulps(kFloor, 1), 0x1p-126, ulps(0x1p-126, -1), 0x1p-125, 1e-30, 1e-7, 0.5, ulps(1.0, -1), 1.0, ulps(1.0, 1), 3.0,
                               1e30, 0x1p127, ulps(kCeil, -1), kCeil};
        const double nums[] = {kNumLow, ulps(kNumLow, 1), 0x1p-893, 1e-200, 1e-30, ulps(1.0, -1), 1.0, ulps(1.0, 1), 1999.9999999, 2e3, 1e150,
                               ulps(kNumHigh, -1)};
        long edge = 0;
        for (double d : dens)
            for (double x : nums)
                for (int s = 0; s < 4; s++) {
                    if (!plane_div_admits(d)) {
                        std::printf("FAIL predicate: den %a refused\n", d);
                        return 1;
                    }
                    if (!check_pair((s & 1) ? -x : x, (s & 2) ? -d : d, edge)) return 1;
                }
        std::printf("pairs: %ld random and %ld edge pairs admitted, five seeds each\n", tested, edge);
        if (tested < (quick ? 100000 : 1000000) || edge != (long)(sizeof(dens) / 8 * sizeof(nums) / 8 * 4)) {
            std::printf("FAIL pairs: too few admitted\n");
            return 1;
        }
        // outside the predicate, on either side, the scaffolding does act for a num of the range: the floor and the ceiling are not idle
        if (plane_div_admits(ulps(kFloor, -1)) || plane_div_admits(ulps(kCeil, 1)) || plane_div_admits(-ulps(kFloor, -1)) ||
            plane_div_admits(-ulps(kCeil, 1))) {
            std::printf("FAIL predicate: admits a den beyond its floor or its ceiling\n");
            return 1;
        }
        if (!scaffolding_acts(kNumLow, 0x1p130) || !scaffolding_acts(ulps(kNumHigh, -1), 0x1p-270)) {
            std::printf("FAIL predicate: the rules' restatement finds nothing to do well outside it\n");
            return 1;
        }
        std::printf("ok predicate\nok function\n");
    }

    // ---- 3: nums below the range
    {
        long n = 0, equal = 0;
        const long n_cases = quick ? 20000 : 200000;
        const double fixed[] = {0.0, -0.0, 5e-324, -5e-324, 0x1p-1074, 0x1.fffffffffffffp-1023, 0x1p-1022, -0x1p-1022, 0x1p-970, 0x1p-969,
                                ulps(kNumLow, -1), -ulps(kNumLow, -1)};
        for (long k = 0; k < n_cases + (long)(sizeof(fixed) / 8) * 64; k++) {
            double x;
            if (k < n_cases) {
                x = (next_u64() & 1) ? from_bits(next_u64() >> 12) : std::ldexp(0.5 + 0.5 * uni(), -894 - (int)(next_u64() % 180));
                if (next_u64() & 1) x = -x;
            } else {
                x = fixed[(k - n_cases) / 64];
            }
            const double d = random_den();
            if (!plane_div_admits(d) || !(std::fabs(x) < kNumLow)) continue;
            n++;
            const double want = x / d, exact = 1.0 / d;
            for (int s = -2; s <= 2; s++) {
                const double got = plane_div_unscaled(x, d, ulps(exact, s));
                if (!(std::fabs(got) < kSmallBound) || !(std::fabs(want) < kSmallBound) || got > kTMin || want > kTMin) {
                    std::printf("FAIL small nums: num %a den %a: %a, num / den %a\n", x, d, got, want);
                    return 1;
                }
                if (s == 0 && bits(got) == bits(want)) equal++;
            }
        }
        std::printf("small nums: %ld pairs, every result below 2^-764 in both forms; %ld bit-equal at the exact seed\n", n, equal);
        if (n < n_cases / 2) {
            std::printf("FAIL small nums: too few admitted\n");
            return 1;
        }
        std::printf("ok small nums\n");
    }

    // ---- 4: the votes on special values of d_a
    {
        const double specials[] = {0.0, -0.0, 5e-324, -5e-324, 0x1p-1022, 1e-300, 0x1p-149, 0x1p-127, ulps(kFloor, -1), kFloor, ulps(kFloor, 1),
                                   -ulps(kFloor, -1), -kFloor, 0x1p-126, 1e-30, 1.0, -1.0, 0.3, 1e30, ulps(kCeil, -1), kCeil, ulps(kCeil, 1),
                                   -kCeil, -ulps(kCeil, 1), 0x1p128, 1e300, inf, -inf, nan};
        long admitted = 0;
        for (double da : specials) {
            const bool want = std::fabs(da) >= kFloor && std::fabs(da) <= kCeil;  // (a NaN fails both)
            if (plane_div_admits(da) != want) {
                std::printf("FAIL votes: the predicate says %d of d_a = %a\n", (int)!want, da);
                return 1;
            }
            for (int axis = kPlaneAxisX; axis <= kPlaneAxisZ; axis++) {
                double d[3] = {0.25, -0.5, 0.125};
                d[axis - 1] = da;
                const double o[3] = {1.0, -2.0, 3.0};
                const bool b = plane_axis_admits_b(axis, o[0], o[1], o[2], d[0], d[1], d[2]);
                // beyond f32's range phase B's other rule (|o.u| finite in f32) refuses first: the vote may be stricter, never laxer
                // (|d_a| >= 1e37 here: o.u is beyond 3e38 with this origin)
                if (b != want && !(want && !b && std::fabs(da) >= 1e37)) {
                    std::printf("FAIL votes: phase B's vote says %d of d_a = %a on axis %d, the predicate %d\n", (int)b, da, axis, (int)want);
                    return 1;
                }
                if (b && !plane_axis_admits(axis, o[0], o[1], o[2], d[0], d[1], d[2])) {
                    std::printf("FAIL votes: phase B's vote admits d_a = %a on axis %d, plane_axis_admits refuses it\n", da, axis);
                    return 1;
                }
                admitted += b;
            }
        }
        // the host's side: the plane's point
        if (!plane_div_point_ok(0.0) || !plane_div_point_ok(-4.0) || !plane_div_point_ok(9.9e149) || plane_div_point_ok(1e150) ||
            plane_div_point_ok(-1e299) || plane_div_point_ok(inf) || plane_div_point_ok(nan)) {
            std::printf("FAIL votes: plane_div_point_ok\n");
            return 1;
        }
        std::printf("votes: %zu special values of d_a on three axes, %ld admitted\n", sizeof(specials) / 8, admitted);
        std::printf("ok votes\n");
    }
    std::printf("all ok\n");
    return 0;
}
