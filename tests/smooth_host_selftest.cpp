// smooth_host_selftest.cpp -- the host half of flux_ctx_set_mesh_normals (flux_amd/csrc/flux_mesh_attr.h), CPU only and linked against
// nothing: the call's refusals, each with its message, and the normalisation of a fixed set of corner normals printed at full
// precision; tests/test_smooth_normals.py recomputes the values with tests/smooth_spec.py.  Two meshes, of 3 and 2 triangles.
#include <cmath>
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
    // mesh 0: 3 triangles x 3 corners -- long, short, tiny, huge and axis-aligned normals
    std::vector<double> in = {
        3.0, 4.0, 12.0,   0.0, 0.0, -2.0,    1e-150, 2e-150, -2e-150,
        1e150, -1e150, 5e149,   0.1, 0.2, 0.3,   -7.0, 0.0, 0.0,
        1.0, 1.0, 1.0,   0.30000000000000004, -0.1, 0.7,   0.0, 1e-8, 0.0,
    };
    std::vector<double> out = {42.0};
    std::string error;
    CHECK(flux::normalize_corner_normals(first, 0, in.data(), 3, out, error));
    CHECK(out.size() == in.size());
    std::printf("in");
    for (double v : in) std::printf(" %.17g", v);
    std::printf("\nout");
    for (double v : out) std::printf(" %.17g", v);
    std::printf("\n");
    for (size_t k = 0; k < out.size(); k += 3) {
        const double nn = (out[k] * out[k] + out[k + 1] * out[k + 1]) + out[k + 2] * out[k + 2];
        CHECK(std::fabs(nn - 1.0) < 1e-15);
    }

    // the refusals: `out` keeps what it held, the message names the mesh and the first offender
    const std::vector<double> kept = out;
    CHECK(!flux::normalize_corner_normals(first, 2, in.data(), 3, out, error) && has(error, "mesh 2 out of range (2 meshes)"));
    CHECK(!flux::normalize_corner_normals({}, 0, in.data(), 3, out, error) && has(error, "mesh 0 out of range (0 meshes)"));
    CHECK(!flux::normalize_corner_normals(first, 1, in.data(), 3, out, error) && has(error, "mesh 1 has 2 triangles, got normals for 3"));
    CHECK(!flux::normalize_corner_normals(first, 0, nullptr, 3, out, error) && has(error, "null pointer"));
    CHECK(!flux::normalize_corner_normals(first, 0, in.data(), 0, out, error) && has(error, "mesh 0 has 3 triangles, got normals for 0"));
    struct Bad { size_t at; double v; const char *where; };
    const Bad bad[] = {{13, nan, "triangle 1, corner 1"}, {26, inf, "triangle 2, corner 2"}, {0, -inf, "triangle 0, corner 0"}};
    for (const Bad &b : bad) {
        std::vector<double> x = in;
        x[b.at] = b.v;
        CHECK(!flux::normalize_corner_normals(first, 0, x.data(), 3, out, error) && has(error, "mesh 0") && has(error, b.where));
    }
    {   // a zero normal, a length that underflows to zero, a length that overflows: the first offender is named
        std::vector<double> x = in;
        x[15] = x[16] = x[17] = 0.0;
        CHECK(!flux::normalize_corner_normals(first, 0, x.data(), 3, out, error) && has(error, "triangle 1, corner 2"));
        x = in;
        x[6] = 1e-170; x[7] = 0.0; x[8] = 0.0;
        CHECK(!flux::normalize_corner_normals(first, 0, x.data(), 3, out, error) && has(error, "triangle 0, corner 2"));
        x = in;
        x[9] = 1e200;
        x[3] = 0.0; x[4] = 0.0; x[5] = 0.0;
        CHECK(!flux::normalize_corner_normals(first, 0, x.data(), 3, out, error) && has(error, "triangle 0, corner 1"));
        x = in;
        x[9] = 1e200;
        CHECK(!flux::normalize_corner_normals(first, 0, x.data(), 3, out, error) && has(error, "triangle 1, corner 0"));
    }
    CHECK(out == kept);

    // clearing: a null pointer with a count of 0 gives an empty table
    CHECK(flux::normalize_corner_normals(first, 1, nullptr, 0, out, error) && out.empty());
    std::printf("all ok\n");
    return 0;
}
