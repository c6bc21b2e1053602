"""The scenes of the smooth-mesh tests (tests/test_smooth_path_spec.py on the CPU, tests/test_gpu_smooth_normals.py on the GPU) and
their references, made once for every test of a session and never written to.

A scene is 12 x 9 pixels: an 8-segment x 6-ring UV sphere of 80 triangles with its exact vertex normals (its quads fuse into
two-triangle leaf records, its pole triangles do not), a two-triangle floor quad with tilted vertex normals, a second, flat mesh
WITHOUT normals, an analytic sphere and plane, and an inverted Emissive environment."""
import copy
import functools
import os

import numpy as np

from conftest import SCENES

WIDTH, HEIGHT, DEPTH = 12, 9, 4
ROOTS = (2, 8, 16)   # sample roots below, at and above one wave a pixel
MESH_MATERIALS = ("Matte", "Glossy", "Reflective", "Dielectric", "Emissive")
# Per (material, root): the job's seed.  tests/test_smooth_path_spec.py demands that no scene used on the GPU takes a decision
# within 1e-9 of its threshold; one that does gets another seed here (RESEEDED[(material, root)]), and the GPU tests exclude nothing.
SEED_BASE = 4100
RESEEDED = {}


def _material(flux, name):
    return {"Matte": flux.MatteData((0.7, 0.6, 0.5), (0.0, 0.0, 0.0), 0.9),
            "Glossy": flux.GlossyReflectiveData(0.8, (0.9, 0.9, 1.0), 50.0),
            "Reflective": flux.ReflectiveData(0.9, (1.0, 0.95, 0.9)),
            "Dielectric": flux.DielectricData(1.5, (0.9, 1.0, 0.95)),
            "Emissive": flux.EmissiveData((0.3, 0.9, 0.4), 2.0)}[name]


def job_seed(material, root):
    return RESEEDED.get((material, root), SEED_BASE + 16 * MESH_MATERIALS.index(material) + root)


def scene(flux, material="Matte", smooth=True):
    """The scene with the UV sphere of `material`; smooth=False: the same meshes without any normals."""
    from flux_amd.procedural import uv_sphere_mesh
    from flux_amd.scene import MeshData
    sd = copy.deepcopy(flux.load_scene(os.path.join(SCENES, "demo1.yml")))
    sd.scene_name = f"smooth_{material}"
    sd.output_settings.image_width, sd.output_settings.image_height, sd.output_settings.pixel_size = WIDTH, HEIGHT, 30.0
    sd.background = (0.0, 0.0, 0.0)
    sd.camera_settings.eye, sd.camera_settings.look_at, sd.camera_settings.up = (0.3, 2.6, -6.5), (0.0, 0.8, 0.0), (0.0, 1.0, 0.0)
    sd.camera_data.zoom_factor, sd.camera_data.view_plane_distance = 1.0, 500.0
    sd.camera_data.focal_distance, sd.camera_data.lens_radius = 7.0, 0.05
    ball = uv_sphere_mesh(8, 6, (-0.4, 1.1, 0.2), 1.1, _material(flux, material), smooth=smooth)
    fv = np.array([[-3.0, 0.0, -3.0], [3.0, 0.0, -3.0], [3.0, 0.0, 3.5], [-3.0, 0.0, 3.5]])
    ft = np.array([[0, 2, 1], [0, 3, 2]], dtype=np.uint32)   # wound so that the facet normal points up
    tilt = np.array([[-0.4, 1.0, -0.3], [0.5, 1.0, -0.2], [0.3, 2.0, 0.6], [-0.2, 0.5, 0.1]])   # not unit: the call normalises
    floor = MeshData(fv, ft, flux.MatteData((0.5, 0.6, 0.7), (0.0, 0.0, 0.0), 0.8), tilt if smooth else None)
    wv = np.array([[1.2, 0.0, 1.5], [2.9, 0.0, 0.4], [2.6, 2.4, 1.6], [1.4, 2.1, 2.4]])
    wall = MeshData(wv, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint32), flux.MatteData((0.8, 0.3, 0.3), (0.0, 0.0, 0.0), 0.9))
    sd.shapes = [flux.SphereData((0.0, 0.0, 0.0), 60.0, flux.EmissiveData((1.0, 0.97, 0.86), 0.8), True),
                 flux.SphereData((-2.3, 0.7, -0.8), 0.7, flux.GlossyReflectiveData(0.6, (1.0, 0.9, 0.8), 100.0), False),
                 flux.PlaneData((0.0, -0.5, 0.0), (0.0, 1.0, 0.0), flux.MatteData((0.4, 0.4, 0.4), (0.0, 0.0, 0.0), 1.0)),
                 ball, floor, wall]
    return sd


def flat_twin(sd):
    """`sd` with every mesh's normals removed"""
    out = copy.deepcopy(sd)
    for s in out.shapes:
        if hasattr(s, "normals"):
            s.normals = None
    return out


@functools.lru_cache(maxsize=None)
def reference(material, root, smooth=True):
    """(scene, seed, SmoothPathSpec with its frame made) of one job"""
    import flux_amd as flux
    import smooth_path_spec
    sd = scene(flux, material, smooth)
    seed = job_seed(material, root)
    spec = smooth_path_spec.SmoothPathSpec(sd, root, DEPTH, seed)
    spec.frame().setflags(write=False)
    return sd, seed, spec


def lone_wall_scene(flux):
    """The flat mesh alone in the light: the environment and, far outside it where no path can get, a smooth sphere -- a context with
    a table whose every shaded triangle is flat."""
    sd = scene(flux, "Matte")
    far = copy.deepcopy(sd.shapes[3])
    far.vertices = far.vertices + np.array([0.0, 500.0, 0.0])
    sd.shapes = [sd.shapes[0], far, sd.shapes[5]]
    return sd


def c_client_scene(flux):
    """The scene tests/smooth_c_client.c fills by hand"""
    from flux_amd.scene import MeshData
    sd = scene(flux, "Glossy")
    dirs = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)
    tris = np.array([[0, 2, 4], [4, 2, 1], [1, 2, 5], [5, 2, 0], [4, 3, 0], [1, 3, 4], [5, 3, 1], [0, 3, 5]], dtype=np.uint32)
    mesh = MeshData(np.array([0.0, 1.0, 0.0]) + 1.25 * dirs, tris, flux.GlossyReflectiveData(0.8, (0.9, 0.9, 1.0), 50.0), 3.0 * dirs)
    sd.shapes = [sd.shapes[0], sd.shapes[2], mesh]
    return sd


DEBUG_RAYS = 2000


def rays_at_meshes(sd, seed):
    """DEBUG_RAYS unit rays from a shell around the scene towards random points of random triangles of the three meshes of `sd`, and
    the sample set and index their paths draw from"""
    import smooth_spec
    rng = np.random.default_rng(seed)
    v0, e1, e2 = (np.concatenate(x) for x in zip(*[smooth_spec.mesh_triangles(s)[:3] for s in sd.shapes[3:]]))
    k = rng.integers(0, len(v0), DEBUG_RAYS)
    u = rng.uniform(0.02, 0.98, DEBUG_RAYS)
    v = rng.uniform(0.02, 0.98, DEBUG_RAYS) * (1.0 - u)
    target = v0[k] + u[:, None] * e1[k] + v[:, None] * e2[k]
    away = rng.normal(size=(DEBUG_RAYS, 3))
    away[:, 1] = np.abs(away[:, 1]) * 0.7 + 0.1
    o = target + away / np.linalg.norm(away, axis=1)[:, None] * rng.uniform(4.0, 9.0, (DEBUG_RAYS, 1))
    d = target - o
    return o, d / np.linalg.norm(d, axis=1)[:, None], int(rng.integers(0, WIDTH)), int(rng.integers(0, 4))


def debug_rays(material):
    import flux_amd as flux
    return rays_at_meshes(scene(flux, material), RESEEDED.get((material, "rays"), SEED_BASE + 500 + MESH_MATERIALS.index(material)))


def traced(spec, rays):
    """(o, d, set, index, radiance [m, 3], first-hit t [m] -- inf on a miss --, margins) of `rays` (rays_at_meshes) through `spec`"""
    o, d, set_index, index = rays
    rad, _, margins, _, first = spec._trace(o, d, np.full(len(o), set_index), np.full(len(o), index))
    t = np.where(first[0] >= 0, first[1], np.inf)
    return o, d, set_index, index, rad, t, margins


@functools.lru_cache(maxsize=None)
def debug_reference(material):
    """traced: debug_rays through the root-2 job's SmoothPathSpec"""
    return traced(reference(material, 2)[2], debug_rays(material))


# the jobs the GPU tests render against the reference: every material at root 2, the Matte and the glass scene at every root
GPU_JOBS = tuple((m, 2) for m in MESH_MATERIALS) + tuple((m, n) for m in ("Matte", "Dielectric") for n in ROOTS[1:])
