// flux_smooth.h -- the host half of flux_ctx_set_mesh_normals (include/flux_abi.h): the call's checks and the
// normalisation of the corner normals.  Plain C++, no HIP call and no device: abi.hip runs it before its first device call, and
// tests/smooth_host_selftest.cpp runs it stand-alone.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace flux {

// doubles per triangle of the call's layout: [3 corners][3]
constexpr size_t kCornerDoubles = 9;

// Checks `corner_normals` ([num_triangles][3][3]) for mesh `mesh` of a context whose meshes start at triangles mesh_first[m]
// (mesh_first.size() = meshes + 1) and writes n / sqrt(n.n) per corner -- IEEE f64 -- to `out`.  num_triangles == 0 with a null pointer
// clears: `out` comes back empty.  Returns true, or false with the refusal in `error`: the mesh, and the first offending triangle and
// corner.  `out` is untouched by a refusal.
inline bool normalize_corner_normals(const std::vector<uint64_t> &mesh_first, uint64_t mesh, const double *corner_normals,
                                     uint64_t num_triangles, std::vector<double> &out, std::string &error) {
    char buf[200];
    const uint64_t meshes = mesh_first.empty() ? 0 : (uint64_t)mesh_first.size() - 1;
    if (mesh >= meshes) {
        std::snprintf(buf, sizeof(buf), "flux_ctx_set_mesh_normals: mesh %llu out of range (%llu meshes)", (unsigned long long)mesh,
                      (unsigned long long)meshes);
        error = buf;
        return false;
    }
    const uint64_t own = mesh_first[(size_t)mesh + 1] - mesh_first[(size_t)mesh];
    const bool clear = corner_normals == nullptr && num_triangles == 0;
    if (!clear && (corner_normals == nullptr || num_triangles != own)) {
        std::snprintf(buf, sizeof(buf), "flux_ctx_set_mesh_normals: mesh %llu has %llu triangles, got normals for %llu%s", (unsigned long long)mesh,
                      (unsigned long long)own, (unsigned long long)num_triangles, corner_normals ? "" : " and a null pointer");
        error = buf;
        return false;
    }
    std::vector<double> normal;
    if (!clear) {
        normal.resize((size_t)own * kCornerDoubles);
        for (uint64_t k = 0; k < own; k++)
            for (int c = 0; c < 3; c++) {
                const double *n = corner_normals + (size_t)k * kCornerDoubles + 3 * c;
                const double nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
                if (!(std::isfinite(n[0]) && std::isfinite(n[1]) && std::isfinite(n[2]) && std::isfinite(nn) && nn > 0.0)) {
                    std::snprintf(buf, sizeof(buf),
                                  "flux_ctx_set_mesh_normals: mesh %llu, triangle %llu, corner %d: normal (%g, %g, %g) must be finite with a "
                                  "finite length > 0",
                                  (unsigned long long)mesh, (unsigned long long)k, c, n[0], n[1], n[2]);
                    error = buf;
                    return false;
                }
                const double len = std::sqrt(nn);
                double *o = normal.data() + (size_t)k * kCornerDoubles + 3 * c;
                o[0] = n[0] / len;
                o[1] = n[1] / len;
                o[2] = n[2] / len;
            }
    }
    out.swap(normal);
    return true;
}

}  // namespace flux
