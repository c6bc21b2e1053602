/* color_c_client.c -- flux_ctx_set_mesh_colors from plain C (include/flux_abi.h and tests/mesh_attr_c_client.h, nothing else): the
 * octahedron with one colour per vertex.  Prints mesh_attr_c_client.h's lines as
 *   plain <hash>     the frame of the fresh context (the material's colour alone)
 *   colored <hash>   the frame after the call
 *   refusals ok      (the message of a bad component names its triangle, corner and channel)
 *   cleared <hash>   the plain one again
 * tests/test_gpu_vertex_colors.py renders the same scene through the Python binding and compares.
 *
 *   color_c_client <sample_root> <seed>
 */
#include "mesh_attr_c_client.h"

static int bad_colors(flux_ctx *ctx, double colors[8][3][3]) {
    double bad[8][3][3];
    int ok = 1;
    memcpy(bad, colors, sizeof bad);
    bad[5][1][0] = -0.25;
    ok &= refused(flux_ctx_set_mesh_colors(ctx, 0, &bad[0][0][0], 8), "mesh 0, triangle 5, corner 1, channel 0");
    memcpy(bad, colors, sizeof bad);
    bad[2][2][1] = NAN;
    ok &= refused(flux_ctx_set_mesh_colors(ctx, 0, &bad[0][0][0], 8), "mesh 0, triangle 2, corner 2, channel 1");
    memcpy(bad, colors, sizeof bad);
    bad[7][0][2] = INFINITY;
    ok &= refused(flux_ctx_set_mesh_colors(ctx, 0, &bad[0][0][0], 8), "mesh 0, triangle 7, corner 0, channel 2");
    memcpy(bad, colors, sizeof bad);
    bad[0][0][0] = 3.5e38; /* finite, above FLT_MAX */
    bad[3][1][1] = -1.0;
    ok &= refused(flux_ctx_set_mesh_colors(ctx, 0, &bad[0][0][0], 8), "mesh 0, triangle 0, corner 0, channel 0");
    memcpy(bad, colors, sizeof bad);
    bad[4][0][1] = -0.0; /* accepted -- and the same colours again */
    if (flux_ctx_set_mesh_colors(ctx, 0, &bad[0][0][0], 8) != FLUX_OK || flux_ctx_set_mesh_colors(ctx, 0, &colors[0][0][0], 8) != FLUX_OK) ok = 0;
    return ok;
}

int main(int argc, char **argv) {
    const double vertex_color[6][3] = {{1.0, 0.2, 0.1}, {0.1, 0.9, 0.2}, {0.9, 0.9, 0.9}, {0.2, 0.2, 0.2}, {0.1, 0.3, 1.0}, {0.8, 0.7, 0.0}};
    double colors[8][3][3];
    for (int t = 0; t < 8; t++)
        for (int k = 0; k < 3; k++)
            for (int a = 0; a < 3; a++) colors[t][k][a] = vertex_color[octa_indices[t][k]][a];
    return run_client(argc, argv, "color_c_client", flux_ctx_set_mesh_colors, "flux_ctx_set_mesh_colors", "colors", colors, "plain", "colored",
                      bad_colors);
}
