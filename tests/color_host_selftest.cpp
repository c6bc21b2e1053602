// color_host_selftest.cpp -- the host half of flux_ctx_set_mesh_colors (flux_amd/csrc/flux_mesh_attr.h), CPU only and linked against
// nothing: the call's refusals, each with its message, and the f32 rounding of a fixed set of corner colours printed at full
// precision; tests/test_vertex_colors.py recomputes the values with tests/color_spec.py.  Two meshes, of 3 and 2 triangles.
#include <cfloat>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../flux_amd/csrc/flux_mesh_attr.h"

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                  \
        }                                                              \
    } while (0)

static bool has(const std::string &s, const char *needle) { return s.find(needle) != std::string::npos; }

int main() {
    const std::vector<uint64_t> first = {0, 3, 5};
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // mesh 0: 3 triangles x 3 corners -- values that are no f32, ties of the rounding (1 + 2^-24 rounds to even, 1 + 3 2^-24 up), a
    // subnormal f32, a value that underflows to 0, -0.0, FLT_MAX itself and the largest double below it
    std::vector<double> in = {
        0.1, 0.2, 0.30000000000000004,   1.0, 0.0, -0.0,   1.00000005960464477539, 1.00000017881393432617, 0.99999997019767761230,
        1e-40, 1e-46, 1e-50,   0.7, 0.6, 0.5,   (double)FLT_MAX, 3.4028234663852883e+38, 1e38,
        2.5, 1000.0, 16777217.0,   0.3333333333333333, 0.6666666666666666, 0.9999999999999999,   5e-324, 0.25, 0.75,
    };
    std::vector<float> out = {42.0f};
    std::string error;
    CHECK(flux::round_corner_colors(first, 0, in.data(), 3, out, error));
    CHECK(out.size() == in.size());
    std::printf("in");
    for (double v : in) std::printf(" %.17g", v);
    std::printf("\nout");
    for (float v : out) std::printf(" %.9g", (double)v);
    std::printf("\n");
    for (float v : out) CHECK(v >= 0.0f && v <= FLT_MAX);

    // the refusals: `out` keeps what it held, the message names the mesh and the first offender
    const std::vector<float> kept = out;
    CHECK(!flux::round_corner_colors(first, 2, in.data(), 3, out, error) && has(error, "mesh 2 out of range (2 meshes)"));
    CHECK(!flux::round_corner_colors({}, 0, in.data(), 3, out, error) && has(error, "mesh 0 out of range (0 meshes)"));
    CHECK(!flux::round_corner_colors(first, 1, in.data(), 3, out, error) && has(error, "mesh 1 has 2 triangles, got colors for 3"));
    CHECK(!flux::round_corner_colors(first, 0, nullptr, 3, out, error) && has(error, "null pointer"));
    CHECK(!flux::round_corner_colors(first, 0, in.data(), 0, out, error) && has(error, "mesh 0 has 3 triangles, got colors for 0"));
    struct Bad { size_t at; double v; const char *where; };
    const Bad bad[] = {{13, nan, "triangle 1, corner 1, channel 1"},
                       {26, inf, "triangle 2, corner 2, channel 2"},
                       {0, -inf, "triangle 0, corner 0, channel 0"},
                       {5, -1e-300, "triangle 0, corner 1, channel 2"},
                       {21, -5e-324, "triangle 2, corner 1, channel 0"},
                       {9, 3.4028234663852889e+38, "triangle 1, corner 0, channel 0"},   // the next double above FLT_MAX
                       {17, 1e300, "triangle 1, corner 2, channel 2"}};
    for (const Bad &b : bad) {
        std::vector<double> x = in;
        x[b.at] = b.v;
        CHECK(!flux::round_corner_colors(first, 0, x.data(), 3, out, error) && has(error, "mesh 0,") && has(error, b.where));
    }
    {   // two offenders: the first is named
        std::vector<double> x = in;
        x[20] = -1.0;
        x[7] = nan;
        CHECK(!flux::round_corner_colors(first, 0, x.data(), 3, out, error) && has(error, "triangle 0, corner 2, channel 1"));
    }
    CHECK(out == kept);

    // clearing: a null pointer with a count of 0 gives an empty table
    CHECK(flux::round_corner_colors(first, 1, nullptr, 0, out, error) && out.empty());
    std::printf("all ok\n");
    return 0;
}
