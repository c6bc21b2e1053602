// The split kernel's reduced first-plane test for an axis-aligned stored normal (flux_amd/csrc/flux_plane_axis.h) against the general
// expressions, CPU only (tests/test_plane_axis.py builds and runs it; the header is the kernel's and the host's own source).
//   usage: plane_axis_selftest [quick]        (quick: a tenth of the random cases and a thinner grid, for the sanitizer build)
// General: num = (p - o).n, den = d.n, t = num / den, each dot product a + b + c of three products in every order of the terms and every
// fusion a compiler may pick for it under `fp contract(fast)`: unfused, both additions fused, either one fused -- 24 forms of num, 24 of
// den (built with -ffp-contract=off: every fused multiply-add here is spelled out).  Reduced: num = p_a - o_a, den = d_a.
//   1. where plane_axis_admits holds, every form of den has the bits of s d_a, every form of num those of s (p_a - o_a) or -- p_a = o_a --
//      is a zero, and t has the reduced t's bits; with p_a = o_a both are zeros (of whatever sign: the scans ask only t > T_MIN);
//   2. over the grid of special values, every input for which ANY pair of forms gives a t that differs from the reduced one in a bit
//      (two zeros off a zero num excepted, as above) is one the predicate refuses;
//   3. the kernel's phase-B vote (plane_axis_admits_b, from the ray in f32) implies the predicate;
//   4. the classifier: the six axis normals with zeros of either sign; nothing else.
// Prints one "ok <name>" per family and "all ok" at the end; exits 1 on the first failure.
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <thread>
#include <vector>

#include "../flux_amd/csrc/flux_plane_axis.h"

using namespace flux;

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
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
static const double kTMin = 0.0005;

// the 24 forms of x0 n0 + x1 n1 + x2 n2
static void dot_forms(const double x[3], const double n[3], double out[24]) {
    static const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    int k = 0;
    for (const auto &p : perm) {
        const double a = x[p[0]], na = n[p[0]], b = x[p[1]], nb = n[p[1]], c = x[p[2]], nc = n[p[2]];
        out[k++] = (a * na + b * nb) + c * nc;
        out[k++] = __builtin_fma(c, nc, __builtin_fma(b, nb, a * na));
        out[k++] = __builtin_fma(c, nc, a * na + b * nb);
        out[k++] = __builtin_fma(b, nb, a * na) + c * nc;
    }
}
// the distinct bit patterns among 24 values
static int distinct(const double v[24], double out[24]) {
    int n = 0;
    for (int k = 0; k < 24; k++) {
        int j = 0;
        while (j < n && bits(out[j]) != bits(v[k])) j++;
        if (j == n) out[n++] = v[k];
    }
    return n;
}

struct Counts {
    long cases = 0, admitted = 0, refused_though_equal = 0, zero_num = 0, vote_b = 0;
};

static bool fail(const char *what, const double n[3], const double p[3], const double o[3], const double d[3], double tg, double tr) {
    std::printf("FAIL %s: n (%a %a %a) p (%a %a %a) o (%a %a %a) d (%a %a %a): general t %a (%016llx), reduced t %a (%016llx)\n", what, n[0],
                n[1], n[2], p[0], p[1], p[2], o[0], o[1], o[2], d[0], d[1], d[2], tg, (unsigned long long)bits(tg), tr,
                (unsigned long long)bits(tr));
    return false;
}

// one ray against one plane whose normal the classifier has put on `axis`
static bool check(int axis, const double n[3], const double p[3], const double o[3], const double d[3], Counts &c) {
    const double diff[3] = {p[0] - o[0], p[1] - o[1], p[2] - o[2]};  // (S.px - r.ox) etc.: one subtraction each in every form
    double numf[24], denf[24], nums[24], dens[24];
    dot_forms(diff, n, numf);
    dot_forms(d, n, denf);
    const int nn = distinct(numf, nums), nd = distinct(denf, dens);
    double num_r, den_r;
    plane_axis_num_den(axis, p[0], p[1], p[2], o[0], o[1], o[2], d[0], d[1], d[2], num_r, den_r);
    const double t_r = num_r / den_r;
    const bool admits = plane_axis_admits(axis, o[0], o[1], o[2], d[0], d[1], d[2]);
    c.cases++;
    // condition 3: the kernel's f32 vote never admits what the predicate refuses
    if (plane_axis_admits_b(axis, o[0], o[1], o[2], d[0], d[1], d[2])) {
        c.vote_b++;
        if (!admits) return fail("the phase-B vote admits a ray the predicate refuses", n, p, o, d, 0.0, t_r);
    }
    bool any_differs = false;
    double t_bad = 0.0;
    for (int i = 0; i < nn; i++)
        for (int j = 0; j < nd; j++) {
            const double t_g = nums[i] / dens[j];
            const bool same = bits(t_g) == bits(t_r) || (num_r == 0.0 && t_g == 0.0 && t_r == 0.0);
            if (!same) {
                any_differs = true;
                t_bad = t_g;
            }
            // what the scans do with t: the same verdict in both forms wherever the predicate admits
            if (admits && (t_g > kTMin) != (t_r > kTMin)) return fail("verdict", n, p, o, d, t_g, t_r);
        }
    if (admits) {
        c.admitted++;
        if (num_r == 0.0) c.zero_num++;
        if (any_differs) return fail("admitted, but a form differs", n, p, o, d, t_bad, t_r);  // conditions 1 and 2
        const double s = n[axis - 1];
        for (int j = 0; j < nd; j++)
            if (bits(dens[j]) != bits(s * den_r)) return fail("den is not s d_a", n, p, o, d, dens[j], s * den_r);
        for (int i = 0; i < nn; i++)
            if (!(bits(nums[i]) == bits(s * num_r) || (num_r == 0.0 && nums[i] == 0.0))) return fail("num is not s (p_a - o_a)", n, p, o, d, nums[i], s * num_r);
    } else if (!any_differs) {
        c.refused_though_equal++;
    }
    return true;
}

static void normals(double out[12][3]) {  // the six axis normals, zeros positive, then the same with zeros negative
    for (int k = 0; k < 12; k++) {
        const double z = k < 6 ? 0.0 : -0.0;
        out[k][0] = out[k][1] = out[k][2] = z;
        out[k][(k % 6) / 2] = (k & 1) ? -1.0 : 1.0;
    }
}

static bool classifier() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    double n[12][3];
    normals(n);
    for (int k = 0; k < 12; k++)
        if (plane_axis_of(n[k][0], n[k][1], n[k][2], 0.0, -4.0, 1e299) != (k % 6) / 2 + 1) return false;
    // mixed zero signs
    if (plane_axis_of(-0.0, 1.0, 0.0, 0, 0, 0) != kPlaneAxisY || plane_axis_of(0.0, -0.0, -1.0, 0, 0, 0) != kPlaneAxisZ) return false;
    const double none[][3] = {{0.6, 0.8, 0.0}, {0.0, 0.8, 0.6}, {0.0, 2.0, 0.0}, {0.0, 1.0, 1e-300}, {5e-324, 1.0, 0.0}, {0.0, 1.0, -5e-324},
                              {0.0, 0.0, 0.0}, {1.0, 1.0, 0.0}, {1.0, 0.0, 1.0}, {0.0, 1.0 + 2.3e-16, 0.0}, {0.0, 1.0 - 1.2e-16, 0.0},
                              {0.0, -2.0, 0.0}, {0.0, nan, 0.0}, {nan, 1.0, 0.0}, {0.0, 1.0, nan}, {0.0, inf, 0.0}, {inf, 1.0, 0.0},
                              {0.0, 0.5, 0.0}, {0.70710678118654752, 0.70710678118654752, 0.0}};
    for (const auto &v : none)
        if (plane_axis_of(v[0], v[1], v[2], 0, 0, 0) != kPlaneAxisNone) return false;
    // the plane's own point: finite and below the range in every component
    if (plane_axis_of(0, 1, 0, inf, 0, 0) || plane_axis_of(0, 1, 0, 0, 0, nan) || plane_axis_of(0, 1, 0, 0, -1e300, 0)) return false;
    // the camera's scalars
    const double good[] = {0.0, -9.0, 5.5, 1.0, 0.0, 0.0, 9.9e59, 1e-300}, bad1[] = {0.0, 1e60}, bad2[] = {0.0, nan}, bad3[] = {-inf, 1.0};
    return plane_axis_camera_ok(good, 8) && !plane_axis_camera_ok(bad1, 2) && !plane_axis_camera_ok(bad2, 2) && !plane_axis_camera_ok(bad3, 2);
}

int main(int argc, char **argv) {
    const bool quick = argc > 1 && std::strcmp(argv[1], "quick") == 0;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    double N[12][3];
    normals(N);

    if (!classifier()) {
        std::printf("FAIL classifier\n");
        return 1;
    }
    std::printf("ok classifier\n");

    // ---- random rays: ordinary magnitudes, origins on the plane, random bit patterns
    {
        Counts c;
        const long n_cases = quick ? 300000 : 3000000;
        for (long k = 0; k < n_cases; k++) {
            const double *n = N[next_u64() % 12];
            const int axis = plane_axis_of(n[0], n[1], n[2], 0, 0, 0);
            double p[3], o[3], d[3];
            const int family = (int)(next_u64() % 4);
            for (int i = 0; i < 3; i++) {
                p[i] = family == 3 ? 0.0 : 200.0 * uni() - 100.0;
                if (family == 0) {  // a scene's rays
                    o[i] = 2000.0 * uni() - 1000.0;
                    d[i] = 2.0 * uni() - 1.0;
                } else if (family == 1) {  // any bit pattern, NaNs and infinities among them
                    o[i] = from_bits(next_u64());
                    d[i] = from_bits(next_u64());
                } else {  // wide magnitudes, origins on or near the plane
                    o[i] = (next_u64() & 1) ? p[i] : p[i] + std::ldexp(uni() - 0.5, (int)(next_u64() % 120) - 100);
                    d[i] = std::ldexp(uni() - 0.5, (int)(next_u64() % 2000) - 1000);
                }
            }
            if (!check(axis, n, p, o, d, c)) return 1;
        }
        std::printf("random rays: %ld cases, %ld admitted (%ld with a zero num), %ld passed the phase-B vote, %ld refused though every form agreed\n",
                    c.cases, c.admitted, c.zero_num, c.vote_b, c.refused_though_equal);
        if (c.admitted < c.cases / 3 || c.zero_num < c.cases / 100 || c.vote_b < c.cases / 10) {
            std::printf("FAIL random rays: too few cases reach the reduced form\n");
            return 1;
        }
        std::printf("ok random rays\n");
    }

    // ---- the grid of special values in every component of o and d
    {
        const double full[] = {0.0, -0.0, 5e-324, -5e-324, 1e-300, -1e-300, 1.0, -1.0, 1e300, -1e300, inf, -inf, nan};
        const double thin[] = {0.0, -0.0, 5e-324, -1e-300, 1.0, -1.0, 1e300, -inf, nan};
        const double *g = quick ? thin : full;
        const int m = quick ? 9 : 13;
        const double points[2][3] = {{0.0, 0.0, 0.0}, {1.0, -1.0, 0.5}};
        // the six normals against both points, their negative-zero forms against the first: 18 planes, dealt to a few threads
        Counts per_plane[18];
        std::atomic<bool> failed(false);
        auto plane = [&](int pn) {
            const double *n = N[pn % 12];
            const double *p = points[pn / 12];
            const int axis = plane_axis_of(n[0], n[1], n[2], p[0], p[1], p[2]);
            for (int i0 = 0; i0 < m && !failed; i0++)
                for (int i1 = 0; i1 < m; i1++)
                    for (int i2 = 0; i2 < m; i2++)
                        for (int i3 = 0; i3 < m; i3++)
                            for (int i4 = 0; i4 < m; i4++)
                                for (int i5 = 0; i5 < m; i5++) {
                                    const double o[3] = {g[i0], g[i1], g[i2]}, d[3] = {g[i3], g[i4], g[i5]};
                                    if (!check(axis, n, p, o, d, per_plane[pn])) {
                                        failed = true;
                                        return;
                                    }
                                }
        };
        const int n_threads = 6;
        std::vector<std::thread> pool;
        for (int w = 0; w < n_threads; w++)
            pool.emplace_back([&, w] {
                for (int pn = w; pn < 18; pn += n_threads) plane(pn);
            });
        for (std::thread &th : pool) th.join();
        if (failed) return 1;
        Counts c;
        for (const Counts &q : per_plane) {
            c.cases += q.cases; c.admitted += q.admitted; c.zero_num += q.zero_num; c.vote_b += q.vote_b;
            c.refused_though_equal += q.refused_though_equal;
        }
        std::printf("special values: %ld cases, %ld admitted (%ld with a zero num), %ld passed the phase-B vote, %ld refused though every form agreed\n",
                    c.cases, c.admitted, c.zero_num, c.vote_b, c.refused_though_equal);
        if (c.admitted == 0 || c.zero_num == 0 || c.vote_b == 0) {
            std::printf("FAIL special values: nothing reaches the reduced form\n");
            return 1;
        }
        std::printf("ok special values\n");
    }
    std::printf("all ok\n");
    return 0;
}
