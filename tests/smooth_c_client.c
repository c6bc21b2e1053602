/* smooth_c_client.c -- flux_ctx_set_mesh_normals from plain C (include/flux_abi.h and tests/mesh_attr_c_client.h, nothing else):
 * the octahedron with its vertex directions as corner normals.  Prints mesh_attr_c_client.h's lines as
 *   flat <hash>      the frame of the fresh context (facet normals)
 *   smooth <hash>    the frame after the call
 *   refusals ok
 *   cleared <hash>   the flat one again
 * tests/test_gpu_smooth_normals.py renders the same scene through the Python binding and compares.
 *
 *   smooth_c_client <sample_root> <seed>
 */
#include "mesh_attr_c_client.h"

static int bad_normals(flux_ctx *ctx, double normals[8][3][3]) {
    double bad[8][3][3];
    int ok = 1;
    memcpy(bad, normals, sizeof bad);
    bad[5][1][0] = bad[5][1][1] = bad[5][1][2] = 0.0;
    ok &= refused(flux_ctx_set_mesh_normals(ctx, 0, &bad[0][0][0], 8), "mesh 0, triangle 5, corner 1");
    memcpy(bad, normals, sizeof bad);
    bad[2][2][1] = NAN;
    ok &= refused(flux_ctx_set_mesh_normals(ctx, 0, &bad[0][0][0], 8), "mesh 0, triangle 2, corner 2");
    memcpy(bad, normals, sizeof bad);
    bad[7][0][2] = INFINITY;
    ok &= refused(flux_ctx_set_mesh_normals(ctx, 0, &bad[0][0][0], 8), "mesh 0, triangle 7, corner 0");
    return ok;
}

int main(int argc, char **argv) {
    double normals[8][3][3];
    for (int t = 0; t < 8; t++)
        for (int k = 0; k < 3; k++)
            for (int a = 0; a < 3; a++) normals[t][k][a] = 3.0 * octa_dir[octa_indices[t][k]][a]; /* (not unit: the call normalises) */
    return run_client(argc, argv, "smooth_c_client", flux_ctx_set_mesh_normals, "flux_ctx_set_mesh_normals", "normals", normals, "flat",
                      "smooth", bad_normals);
}
