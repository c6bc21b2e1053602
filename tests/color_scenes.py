"""The scenes of the vertex-colour tests (tests/test_color_path_spec.py on the CPU, tests/test_gpu_vertex_colors.py on the GPU) and
their references, made once for every test of a session and never written to.

The scene is tests/smooth_scenes.py's 12 x 9 scene with other attributes on its three meshes: the 80-triangle UV sphere has its
normals AND per-vertex colours, the two-triangle floor has a per-corner checker and NO normals, the wall has neither.  The corner
colours of every coloured triangle differ by at least 0.3 in some channel, so a swapped or dropped corner moves a sample by as much;
one palette entry has a zero channel."""
import copy
import functools

import numpy as np

import smooth_scenes

WIDTH, HEIGHT, DEPTH, ROOTS = smooth_scenes.WIDTH, smooth_scenes.HEIGHT, smooth_scenes.DEPTH, smooth_scenes.ROOTS
MESH_MATERIALS = smooth_scenes.MESH_MATERIALS
# Per (material, root): the job's seed.  tests/test_color_path_spec.py demands that no scene used on the GPU takes a decision within
# 1e-9 of its threshold; one that does gets another seed here, and the GPU tests exclude nothing.
SEED_BASE = 5200
RESEEDED = {}

PALETTE = np.array([[1.0, 0.3, 0.0], [0.2, 0.9, 0.3], [0.3, 0.4, 1.0]])
FLOOR_CHECKER = np.array([[[0.9, 0.9, 0.8], [0.2, 0.2, 0.3], [0.9, 0.5, 0.2]],
                          [[0.1, 0.3, 0.9], [0.9, 0.9, 0.9], [0.2, 0.8, 0.3]]])


def job_seed(material, root):
    return RESEEDED.get((material, root), SEED_BASE + 16 * MESH_MATERIALS.index(material) + root)


def sphere_colors(segments=8, rings=6):
    """Per-vertex colours [42][3] of uv_sphere_mesh(8, 6): the poles white and dark, vertex (ring r, segment s) PALETTE[(r + s) % 3]
    -- the corners of every triangle then hold at least two palette entries"""
    out = [[1.0, 1.0, 1.0]]
    for r in range(rings - 1):
        for s in range(segments):
            out.append(PALETTE[(r + s) % 3])
    out.append([0.1, 0.1, 0.15])
    return np.array(out, dtype=np.float64)


def scene(flux, material="Matte", colors="on", normals=True):
    """colors: "on" (the sphere per vertex, the floor per corner), "ones" (all-ones colours on every mesh, the wall included) or
    None; normals: the sphere's (the floor never has any here)"""
    sd = smooth_scenes.scene(flux, material, smooth=normals)
    sd.scene_name = f"color_{material}"
    ball, floor, wall = sd.shapes[3], sd.shapes[4], sd.shapes[5]
    floor.normals = None
    if colors == "on":
        ball.colors, floor.colors = sphere_colors(), FLOOR_CHECKER.copy()
    elif colors == "ones":
        for m in (ball, floor, wall):
            m.colors = np.ones((len(m.triangles), 3, 3))
    return sd


def spread(mesh):
    """the smallest, over the mesh's triangles, of the largest difference between two corners in one channel"""
    from flux_amd.scene import corner_colors
    c = corner_colors(mesh)
    return float((c.max(axis=1) - c.min(axis=1)).max(axis=1).min())


@functools.lru_cache(maxsize=None)
def reference(material, root, colors="on"):
    """(scene, seed, ColorPathSpec with its frame made) of one job"""
    import flux_amd as flux
    import color_path_spec
    sd = scene(flux, material, colors)
    seed = job_seed(material, root)
    spec = color_path_spec.ColorPathSpec(sd, root, DEPTH, seed)
    spec.frame().setflags(write=False)
    return sd, seed, spec


def c_client_scene(flux):
    """The scene tests/color_c_client.c fills by hand: smooth_scenes.c_client_scene's octahedron without normals, its six vertices
    coloured"""
    sd = smooth_scenes.c_client_scene(flux)
    mesh = sd.shapes[2]
    mesh.normals = None
    mesh.colors = np.array([[1.0, 0.2, 0.1], [0.1, 0.9, 0.2], [0.9, 0.9, 0.9], [0.2, 0.2, 0.2], [0.1, 0.3, 1.0], [0.8, 0.7, 0.0]])
    return sd


def plain_twin(sd):
    """`sd` with every mesh's colours removed"""
    out = copy.deepcopy(sd)
    for s in out.shapes:
        if hasattr(s, "colors"):
            s.colors = None
    return out


def debug_rays(material):
    """smooth_scenes.rays_at_meshes on this scene's meshes, with this file's seeds"""
    import flux_amd as flux
    return smooth_scenes.rays_at_meshes(scene(flux, material), RESEEDED.get((material, "rays"), SEED_BASE + 500 + MESH_MATERIALS.index(material)))


@functools.lru_cache(maxsize=None)
def debug_reference(material):
    """smooth_scenes.traced: debug_rays through the root-2 job's ColorPathSpec"""
    return smooth_scenes.traced(reference(material, 2)[2], debug_rays(material))


# the jobs the GPU tests render against the reference: every material at root 2, the Matte and the glass scene at every root
GPU_JOBS = tuple((m, 2) for m in MESH_MATERIALS) + tuple((m, n) for m in ("Matte", "Dielectric") for n in ROOTS[1:])
