// flux_color.h -- the host half of flux_ctx_set_mesh_colors (include/flux_abi.h): the call's checks and the
// rounding of the corner colours to f32.  Plain C++, no HIP call and no device: abi.hip runs it before its first device call, and
// tests/color_host_selftest.cpp runs it stand-alone.
#pragma once
#include <cfloat>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "flux_smooth.h"  // kCornerDoubles: the two calls share the layout [triangles][3 corners][3]

namespace flux {

// Checks `corner_colors` ([num_triangles][3 corners][3 rgb]) for mesh `mesh` of a context whose meshes start at triangles
// mesh_first[m] (mesh_first.size() = meshes + 1) and writes (float)x per component -- round to nearest even -- to `out`.  A component
// x is accepted iff x >= 0 and x <= FLT_MAX (so -0.0 is, a NaN, a negative value, an infinity and anything that would round to one
// are not).  num_triangles == 0 with a null pointer clears: `out` comes back empty.  Returns true, or false with the refusal in
// `error`: the mesh, and the first offending triangle, corner and channel.  `out` is untouched by a refusal.
inline bool round_corner_colors(const std::vector<uint64_t> &mesh_first, uint64_t mesh, const double *corner_colors, uint64_t num_triangles,
                                std::vector<float> &out, std::string &error) {
    char buf[240];
    const uint64_t meshes = mesh_first.empty() ? 0 : (uint64_t)mesh_first.size() - 1;
    if (mesh >= meshes) {
        std::snprintf(buf, sizeof(buf), "flux_ctx_set_mesh_colors: mesh %llu out of range (%llu meshes)", (unsigned long long)mesh,
                      (unsigned long long)meshes);
        error = buf;
        return false;
    }
    const uint64_t own = mesh_first[(size_t)mesh + 1] - mesh_first[(size_t)mesh];
    const bool clear = corner_colors == nullptr && num_triangles == 0;
    if (!clear && (corner_colors == nullptr || num_triangles != own)) {
        std::snprintf(buf, sizeof(buf), "flux_ctx_set_mesh_colors: mesh %llu has %llu triangles, got colors for %llu%s", (unsigned long long)mesh,
                      (unsigned long long)own, (unsigned long long)num_triangles, corner_colors ? "" : " and a null pointer");
        error = buf;
        return false;
    }
    std::vector<float> color;
    if (!clear) {
        color.resize((size_t)own * kCornerDoubles);
        for (uint64_t k = 0; k < own; k++)
            for (int c = 0; c < 3; c++)
                for (int ch = 0; ch < 3; ch++) {
                    const size_t at = (size_t)k * kCornerDoubles + 3 * c + ch;
                    const double x = corner_colors[at];
                    if (!(x >= 0.0 && x <= (double)FLT_MAX)) {
                        std::snprintf(buf, sizeof(buf),
                                      "flux_ctx_set_mesh_colors: mesh %llu, triangle %llu, corner %d, channel %d: component %g must lie in "
                                      "[0, FLT_MAX]",
                                      (unsigned long long)mesh, (unsigned long long)k, c, ch, x);
                        error = buf;
                        return false;
                    }
                    color[at] = (float)x;
                }
    }
    out.swap(color);
    return true;
}

}  // namespace flux
