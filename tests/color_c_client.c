/* color_c_client.c -- flux_ctx_set_mesh_colors from plain C (include/flux_abi.h and nothing else): an octahedron with one colour
 * per vertex over a Matte plane inside an Emissive environment, 12 x 9 pixels.  Prints, one per line:
 *   plain <hash>     the frame of the fresh context (the material's colour alone)
 *   colored <hash>   the frame after the call
 *   refusals ok      every refusal of the header returned FLUX_E_INVALID with a message naming the mesh (and the triangle, corner
 *                    and channel of a bad component), and the frame after them is still the coloured one
 *   cleared <hash>   the frame after clearing: the plain one again
 * <hash> is FNV-1a (64 bit) over the frame's bytes; tests/test_gpu_vertex_colors.py renders the same scene through the Python
 * binding and compares.
 *
 *   color_c_client <sample_root> <seed>
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "flux_abi.h"

#define W 12
#define H 9

static unsigned long long fnv1a(const void *data, size_t bytes) {
    const unsigned char *p = (const unsigned char *)data;
    unsigned long long h = 1469598103934665603ull;
    for (size_t k = 0; k < bytes; k++) {
        h ^= p[k];
        h *= 1099511628211ull;
    }
    return h;
}

static int refused(int rc, const char *needle) {
    if (rc != FLUX_E_INVALID || !strstr(flux_last_error(), needle)) {
        fprintf(stderr, "expected FLUX_E_INVALID with \"%s\", got %d: %s\n", needle, rc, flux_last_error());
        return 0;
    }
    return 1;
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s sample_root seed\n", argv[0]);
        return 2;
    }
    flux_job_cfg cfg;
    cfg.sample_root = strtoull(argv[1], NULL, 10);
    cfg.max_trace_depth = 4;
    cfg.rows_per_work_unit = 50;
    const uint64_t seed = strtoull(argv[2], NULL, 10);

    flux_shape shapes[2];
    memset(shapes, 0, sizeof shapes);
    shapes[0].kind = FLUX_SHAPE_SPHERE;
    shapes[0].invert = 1;
    shapes[0].radius = 60.0;
    shapes[0].material.kind = FLUX_MAT_EMISSIVE;
    shapes[0].material.color[0] = 1.0; shapes[0].material.color[1] = 0.97; shapes[0].material.color[2] = 0.86;
    shapes[0].material.k = 0.8;
    shapes[1].kind = FLUX_SHAPE_PLANE;
    shapes[1].p[1] = -0.5;
    shapes[1].n[1] = 1.0;
    shapes[1].material.kind = FLUX_MAT_MATTE;
    shapes[1].material.color[0] = shapes[1].material.color[1] = shapes[1].material.color[2] = 0.4;
    shapes[1].material.k = 1.0;

    /* the octahedron: +x, -x, +y, -y, +z, -z around (0, 1, 0), radius 1.25; triangles wound outwards */
    const double c[3] = {0.0, 1.0, 0.0}, r = 1.25;
    const double dir[6][3] = {{1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}};
    double vertices[6][3];
    for (int k = 0; k < 6; k++)
        for (int a = 0; a < 3; a++) vertices[k][a] = c[a] + r * dir[k][a];
    const uint32_t indices[8][3] = {{0, 2, 4}, {4, 2, 1}, {1, 2, 5}, {5, 2, 0}, {4, 3, 0}, {1, 3, 4}, {5, 3, 1}, {0, 3, 5}};
    const double vertex_color[6][3] = {{1.0, 0.2, 0.1}, {0.1, 0.9, 0.2}, {0.9, 0.9, 0.9}, {0.2, 0.2, 0.2}, {0.1, 0.3, 1.0}, {0.8, 0.7, 0.0}};
    double colors[8][3][3];
    for (int t = 0; t < 8; t++)
        for (int k = 0; k < 3; k++)
            for (int a = 0; a < 3; a++) colors[t][k][a] = vertex_color[indices[t][k]][a];
    flux_mesh mesh;
    memset(&mesh, 0, sizeof mesh);
    mesh.num_vertices = 6;
    mesh.vertices = &vertices[0][0];
    mesh.num_triangles = 8;
    mesh.indices = &indices[0][0];
    mesh.material.kind = FLUX_MAT_GLOSSY;
    mesh.material.color[0] = 0.9; mesh.material.color[1] = 0.9; mesh.material.color[2] = 1.0;
    mesh.material.k = 0.8;
    mesh.material.exponent = 50.0;

    flux_scene_desc scene;
    memset(&scene, 0, sizeof scene);
    scene.scene_name = "color_c_client";
    scene.image_width = W;
    scene.image_height = H;
    scene.pixel_size = 30.0;
    scene.eye[0] = 0.3; scene.eye[1] = 2.6; scene.eye[2] = -6.5;
    scene.look_at[1] = 0.8;
    scene.up[1] = 1.0;
    scene.zoom_factor = 1.0;
    scene.view_plane_distance = 500.0;
    scene.focal_distance = 7.0;
    scene.lens_radius = 0.05;
    scene.num_shapes = 2;
    scene.shapes = shapes;
    scene.num_meshes = 1;
    scene.meshes = &mesh;

    /* without a context */
    if (!refused(flux_ctx_set_mesh_colors(NULL, 0, &colors[0][0][0], 8), "null context")) return 1;

    flux_ctx *ctx = NULL;
    if (flux_ctx_create(&scene, &cfg, seed, 0, &ctx) != FLUX_OK) {
        fprintf(stderr, "flux_ctx_create: %s\n", flux_last_error());
        return 1;
    }
    static double plain[H][W][3], colored[H][W][3], again[H][W][3];
    const uint64_t bytes0 = flux_ctx_device_bytes(ctx);
    if (flux_render_rows(ctx, 0, H - 1, &plain[0][0][0]) != FLUX_OK) return 1;
    printf("plain %016llx\n", fnv1a(plain, sizeof plain));

    if (flux_ctx_set_mesh_colors(ctx, 0, &colors[0][0][0], 8) != FLUX_OK) {
        fprintf(stderr, "flux_ctx_set_mesh_colors: %s\n", flux_last_error());
        return 1;
    }
    if (flux_ctx_device_bytes(ctx) != bytes0 + 8 * 128) {
        fprintf(stderr, "device bytes %llu, expected %llu\n", (unsigned long long)flux_ctx_device_bytes(ctx), (unsigned long long)(bytes0 + 8 * 128));
        return 1;
    }
    if (flux_render_rows(ctx, 0, H - 1, &colored[0][0][0]) != FLUX_OK) return 1;
    printf("colored %016llx\n", fnv1a(colored, sizeof colored));

    /* the refusals, on the live context */
    double bad[8][3][3];
    int ok = 1;
    ok &= refused(flux_ctx_set_mesh_colors(ctx, 1, &colors[0][0][0], 8), "mesh 1 out of range (1 meshes)");
    ok &= refused(flux_ctx_set_mesh_colors(ctx, 0, &colors[0][0][0], 7), "mesh 0 has 8 triangles, got colors for 7");
    ok &= refused(flux_ctx_set_mesh_colors(ctx, 0, NULL, 8), "mesh 0 has 8 triangles");
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
    if (!ok) return 1;
    if (flux_ctx_device_bytes(ctx) != bytes0 + 8 * 128) return 1;
    if (flux_render_rows(ctx, 0, H - 1, &again[0][0][0]) != FLUX_OK || memcmp(again, colored, sizeof colored) != 0) {
        fprintf(stderr, "the context changed under a refused call\n");
        return 1;
    }
    printf("refusals ok\n");

    if (flux_ctx_set_mesh_colors(ctx, 0, NULL, 0) != FLUX_OK || flux_ctx_device_bytes(ctx) != bytes0) return 1;
    if (flux_render_rows(ctx, 0, H - 1, &again[0][0][0]) != FLUX_OK) return 1;
    printf("cleared %016llx\n", fnv1a(again, sizeof again));
    flux_ctx_destroy(ctx);
    return 0;
}
