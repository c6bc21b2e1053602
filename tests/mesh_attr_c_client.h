/* mesh_attr_c_client.h -- what tests/smooth_c_client.c and tests/color_c_client.c share: a per-mesh attribute call of
 * include/flux_abi.h from plain C, on an octahedron over a Matte plane inside an Emissive environment, 12 x 9 pixels.  A client
 * fills the attribute's values [8][3][3] from octa_dir / octa_indices, names its call and its lines, and hands run_client its own
 * bad-value cases.  run_client prints, one per line:
 *   <before> <hash>  the frame of the fresh context
 *   <after> <hash>   the frame after the call
 *   refusals ok      every refusal of the header returned FLUX_E_INVALID with a message naming the mesh, and the frame after them
 *                    is still the one after the call
 *   cleared <hash>   the frame after clearing: the first one again
 * <hash> is FNV-1a (64 bit) over the frame's bytes; the GPU suites render the same scene through the Python binding and compare.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "flux_abi.h"

#define W 12
#define H 9

/* the octahedron: +x, -x, +y, -y, +z, -z around (0, 1, 0), radius 1.25; triangles wound outwards */
static const double octa_dir[6][3] = {{1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}};
static const uint32_t octa_indices[8][3] = {{0, 2, 4}, {4, 2, 1}, {1, 2, 5}, {5, 2, 0}, {4, 3, 0}, {1, 3, 4}, {5, 3, 1}, {0, 3, 5}};

typedef int (*set_mesh_attr)(flux_ctx *ctx, uint64_t mesh, const double *corners, uint64_t num_triangles);

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

/* The client's main: `set` is the call, `call` its name, `what` its noun in the refusals ("normals"), `values` the attribute;
 * `bad_values(ctx, values)` runs the client's bad-value cases on the live context and returns 1 iff each went as it should. */
static int run_client(int argc, char **argv, const char *scene_name, set_mesh_attr set, const char *call, const char *what,
                      double values[8][3][3], const char *before, const char *after, int (*bad_values)(flux_ctx *, double[8][3][3])) {
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

    const double c[3] = {0.0, 1.0, 0.0}, r = 1.25;
    double vertices[6][3];
    for (int k = 0; k < 6; k++)
        for (int a = 0; a < 3; a++) vertices[k][a] = c[a] + r * octa_dir[k][a];
    flux_mesh mesh;
    memset(&mesh, 0, sizeof mesh);
    mesh.num_vertices = 6;
    mesh.vertices = &vertices[0][0];
    mesh.num_triangles = 8;
    mesh.indices = &octa_indices[0][0];
    mesh.material.kind = FLUX_MAT_GLOSSY;
    mesh.material.color[0] = 0.9; mesh.material.color[1] = 0.9; mesh.material.color[2] = 1.0;
    mesh.material.k = 0.8;
    mesh.material.exponent = 50.0;

    flux_scene_desc scene;
    memset(&scene, 0, sizeof scene);
    scene.scene_name = scene_name;
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
    if (!refused(set(NULL, 0, &values[0][0][0], 8), "null context")) return 1;

    flux_ctx *ctx = NULL;
    if (flux_ctx_create(&scene, &cfg, seed, 0, &ctx) != FLUX_OK) {
        fprintf(stderr, "flux_ctx_create: %s\n", flux_last_error());
        return 1;
    }
    static double fresh[H][W][3], with[H][W][3], again[H][W][3];
    const uint64_t bytes0 = flux_ctx_device_bytes(ctx);
    if (flux_render_rows(ctx, 0, H - 1, &fresh[0][0][0]) != FLUX_OK) return 1;
    printf("%s %016llx\n", before, fnv1a(fresh, sizeof fresh));

    if (set(ctx, 0, &values[0][0][0], 8) != FLUX_OK) {
        fprintf(stderr, "%s: %s\n", call, flux_last_error());
        return 1;
    }
    if (flux_ctx_device_bytes(ctx) != bytes0 + 8 * 128) {
        fprintf(stderr, "device bytes %llu, expected %llu\n", (unsigned long long)flux_ctx_device_bytes(ctx), (unsigned long long)(bytes0 + 8 * 128));
        return 1;
    }
    if (flux_render_rows(ctx, 0, H - 1, &with[0][0][0]) != FLUX_OK) return 1;
    printf("%s %016llx\n", after, fnv1a(with, sizeof with));

    /* the refusals, on the live context */
    char wrong_count[80];
    snprintf(wrong_count, sizeof wrong_count, "mesh 0 has 8 triangles, got %s for 7", what);
    int ok = 1;
    ok &= refused(set(ctx, 1, &values[0][0][0], 8), "mesh 1 out of range (1 meshes)");
    ok &= refused(set(ctx, 0, &values[0][0][0], 7), wrong_count);
    ok &= refused(set(ctx, 0, NULL, 8), "mesh 0 has 8 triangles");
    ok &= bad_values(ctx, values);
    if (!ok) return 1;
    if (flux_ctx_device_bytes(ctx) != bytes0 + 8 * 128) return 1;
    if (flux_render_rows(ctx, 0, H - 1, &again[0][0][0]) != FLUX_OK || memcmp(again, with, sizeof with) != 0) {
        fprintf(stderr, "the context changed under a refused call\n");
        return 1;
    }
    printf("refusals ok\n");

    if (set(ctx, 0, NULL, 0) != FLUX_OK || flux_ctx_device_bytes(ctx) != bytes0) return 1;
    if (flux_render_rows(ctx, 0, H - 1, &again[0][0][0]) != FLUX_OK) return 1;
    printf("cleared %016llx\n", fnv1a(again, sizeof again));
    flux_ctx_destroy(ctx);
    return 0;
}
