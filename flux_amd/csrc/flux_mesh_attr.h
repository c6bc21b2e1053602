// flux_mesh_attr.h -- the host half of flux_ctx_set_mesh_normals and flux_ctx_set_mesh_colors (include/flux_abi.h, DESIGN.md sections
// 5j and 5k): the checks the two calls share, the normalisation of the corner normals and the rounding of the corner colours to f32.
// Plain C++, no HIP call and no device: abi.hip runs it before its first device call, and tests/smooth_host_selftest.cpp and
// tests/color_host_selftest.cpp run it stand-alone.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace flux {

// doubles per triangle of the calls' layout: [3 corners][3]
constexpr size_t kCornerDoubles = 9;

// What every per-mesh attribute call checks alike, for `call` ("flux_ctx_set_mesh_normals") and its noun `what` ("normals"): mesh
// `mesh` of a context whose meshes start at triangles mesh_first[m] (mesh_first.size() = meshes + 1), `num_triangles` against the
// mesh's own count, the null pointer.  num_triangles == 0 with a null pointer clears.  Returns true with the mesh's count in `own`
// and the clear case in `clear`, or false with the refusal in `error`.
inline bool check_mesh_attribute(const char *call, const char *what, const std::vector<uint64_t> &mesh_first, uint64_t mesh,
                                 const double *corners, uint64_t num_triangles, uint64_t &own, bool &clear, std::string &error) {
    char buf[240];
    const uint64_t meshes = mesh_first.empty() ? 0 : (uint64_t)mesh_first.size() - 1;
    if (mesh >= meshes) {
        std::snprintf(buf, sizeof(buf), "%s: mesh %llu out of range (%llu meshes)", call, (unsigned long long)mesh, (unsigned long long)meshes);
        error = buf;
        return false;
    }
    own = mesh_first[(size_t)mesh + 1] - mesh_first[(size_t)mesh];
    clear = corners == nullptr && num_triangles == 0;
    if (!clear && (corners == nullptr || num_triangles != own)) {
        std::snprintf(buf, sizeof(buf), "%s: mesh %llu has %llu triangles, got %s for %llu%s", call, (unsigned long long)mesh,
                      (unsigned long long)own, what, (unsigned long long)num_triangles, corners ? "" : " and a null pointer");
        error = buf;
        return false;
    }
    return true;
}

// Checks `corner_normals` ([num_triangles][3][3]) by check_mesh_attribute and writes n / sqrt(n.n) per corner -- IEEE f64 -- to `out`;
// a clear leaves `out` empty.  Returns true, or false with the refusal in `error`: the mesh, and the first offending triangle and
// corner.  `out` is untouched by a refusal.
inline bool normalize_corner_normals(const std::vector<uint64_t> &mesh_first, uint64_t mesh, const double *corner_normals,
                                     uint64_t num_triangles, std::vector<double> &out, std::string &error) {
    uint64_t own;
    bool clear;
    if (!check_mesh_attribute("flux_ctx_set_mesh_normals", "normals", mesh_first, mesh, corner_normals, num_triangles, own, clear, error))
        return false;
    std::vector<double> normal(clear ? 0 : (size_t)own * kCornerDoubles);
    for (size_t at = 0; at < normal.size(); at += 3) {
        const double *n = corner_normals + at;
        const double nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
        if (!(std::isfinite(n[0]) && std::isfinite(n[1]) && std::isfinite(n[2]) && std::isfinite(nn) && nn > 0.0)) {
            char buf[200];
            std::snprintf(buf, sizeof(buf),
                          "flux_ctx_set_mesh_normals: mesh %llu, triangle %llu, corner %d: normal (%g, %g, %g) must be finite with a "
                          "finite length > 0",
                          (unsigned long long)mesh, (unsigned long long)(at / kCornerDoubles), (int)(at % kCornerDoubles / 3), n[0], n[1], n[2]);
            error = buf;
            return false;
        }
        const double len = std::sqrt(nn);
        normal[at] = n[0] / len;
        normal[at + 1] = n[1] / len;
        normal[at + 2] = n[2] / len;
    }
    out.swap(normal);
    return true;
}

// Checks `corner_colors` ([num_triangles][3 corners][3 rgb]) by check_mesh_attribute and writes (float)x per component -- round to
// nearest even -- to `out`; a clear leaves `out` empty.  A component x is accepted iff x >= 0 and x <= FLT_MAX (so -0.0 is, a NaN, a
// negative value, an infinity and anything that would round to one are not).  Returns true, or false with the refusal in `error`:
// the mesh, and the first offending triangle, corner and channel.  `out` is untouched by a refusal.
inline bool round_corner_colors(const std::vector<uint64_t> &mesh_first, uint64_t mesh, const double *corner_colors, uint64_t num_triangles,
                                std::vector<float> &out, std::string &error) {
    uint64_t own;
    bool clear;
    if (!check_mesh_attribute("flux_ctx_set_mesh_colors", "colors", mesh_first, mesh, corner_colors, num_triangles, own, clear, error))
        return false;
    std::vector<float> color(clear ? 0 : (size_t)own * kCornerDoubles);
    for (size_t at = 0; at < color.size(); at++) {
        const double x = corner_colors[at];
        if (!(x >= 0.0 && x <= (double)FLT_MAX)) {
            char buf[240];
            std::snprintf(buf, sizeof(buf),
                          "flux_ctx_set_mesh_colors: mesh %llu, triangle %llu, corner %d, channel %d: component %g must lie in "
                          "[0, FLT_MAX]",
                          (unsigned long long)mesh, (unsigned long long)(at / kCornerDoubles), (int)(at % kCornerDoubles / 3), (int)(at % 3), x);
            error = buf;
            return false;
        }
        color[at] = (float)x;
    }
    out.swap(color);
    return true;
}

}  // namespace flux
