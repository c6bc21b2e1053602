// aov_host_selftest.cpp -- flux_host::aov_image (flux_amd/host/flux_host.hpp) on a small fixed feature buffer, CPU only: prints the
// buffer and the image of each of the four kinds at full precision; tests/test_aov.py compares them with the numpy mapping of
// tests/aov_spec.py.  The buffer holds the cases the mapping singles out: a zero normal, a non-unit normal, an infinite depth, an
// albedo above 1, a pixel nothing covers and a partly covered one.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../flux_amd/host/flux_host.hpp"

using namespace flux_host;

int main() {
    const size_t w = 3, h = 2;
    const double inf = std::numeric_limits<double>::infinity();
    // albedo (3), normal (3), depth, coverage
    const double px[w * h][FLUX_AOV_CHANNELS] = {
        {0.72, 0.54, 0.36, 0.0, 0.6, -0.8, 5.25, 1.0},        // a unit normal
        {3.0, 2.7, 2.4, 0.1, -0.2, 0.05, 7.5, 0.640625},      // albedo above 1, a short mean normal, partly covered
        {0.1, 0.2, 0.3, 0.0, 0.0, 0.0, 0.0, 0.0},             // nothing hit: the zero normal
        {0.72, 0.72, 0.72, 0.0, 1.0, 0.0, inf, 1.0},          // a plane seen along its horizon: depth +inf
        {0.5, 1.0, 1.0000000000000002, -1.0, 0.0, 0.0, 110.0, 1.0},  // the farthest finite depth
        {0.0, 0.0, 0.0, 3.0, 4.0, 12.0, 0.0005, 0.015625},    // a non-unit stored normal, nearly uncovered
    };
    std::vector<double> aov;
    for (const auto &p : px)
        for (double v : p) aov.push_back(v);
    std::printf("size %zu %zu\n", w, h);
    std::printf("aov");
    for (double v : aov) std::printf(" %.17g", v);
    std::printf("\n");
    const struct { AovKind kind; const char *name; } kinds[] = {
        {AovKind::Albedo, "albedo"}, {AovKind::Normal, "normal"}, {AovKind::Depth, "depth"}, {AovKind::Coverage, "coverage"}};
    for (const auto &k : kinds) {
        const std::vector<double> img = aov_image(aov.data(), w, h, k.kind);
        if (img.size() != w * h * 3) return 1;
        std::printf("%s", k.name);
        for (double v : img) {
            if (!(v >= 0.0 && v <= 1.0)) return 2;  // the image is in [0, 1], whatever the buffer holds
            std::printf(" %.17g", v);
        }
        std::printf("\n");
    }
    // a frame without any finite depth above 0: t_max falls back to 1
    const double flat[FLUX_AOV_CHANNELS] = {0.1, 0.2, 0.3, 0.0, 0.0, 0.0, 0.0, 0.0};
    const std::vector<double> img = aov_image(flat, 1, 1, AovKind::Depth);
    std::printf("flat %.17g %.17g %.17g\n", img[0], img[1], img[2]);
    std::printf("all ok\n");
    return 0;
}
