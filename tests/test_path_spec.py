"""tests/path_spec.py, the full-path reference of the extension fuzz (tests/test_gpu_ext_fuzz.py), pinned on the CPU before it
judges a kernel: against the restatement on scenes it knows (statistics equal, frames within 1e-12, the project's bound for the
same samples in another summation order, tests/test_gpu_parity.py), against the restatement with boxes as 12-triangle cubes and
disks as planes, by two properties of the Dielectric spec, and -- for the fuzz's own scenes -- by the margin of every decision it
took and the number of segments per class.  No GPU."""
import collections
import copy

import numpy as np
import pytest

import box_spec
import path_spec
import test_gpu_ext_fuzz as ext
from conftest import small_scene
from extension_checks import box_as_mesh
from test_box_scene import C0, C1, spec_rays
from test_gpu_fuzz import random_scene

SAME_SAMPLES = 1e-12
MARGIN = 1e-9


def against_the_oracle(flux, oracle_mod, sd, n, D, seed, oracle_sd=None, bit_equal=False):
    """PathSpec on `sd` against the restatement on `oracle_sd` (default: the same scene): (largest difference, the PathSpec)."""
    o = oracle_mod.Oracle(oracle_sd or sd, flux.JobConfiguration(n, D, 50), seed=seed)
    o.stats(reset=True)
    want = o.render_frame(threads=4)
    ost = o.stats()
    o.close()
    spec = path_spec.PathSpec(sd, n, D, seed)
    got = spec.frame()
    assert {k: spec.stats[k] for k in ost} == ost
    assert spec.stats["dielectric_reflections"] == spec.stats["dielectric_transmissions"] == 0
    finite = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), finite)
    if bit_equal:
        assert np.array_equal(got, want, equal_nan=True)
    err = float(np.abs(got[finite] - want[finite]).max()) if finite.any() else 0.0
    assert err <= SAME_SAMPLES
    return err, spec


# ---- scenes the restatement knows -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["demo1", "demo2"])
def test_demo_scenes(flux, oracle_mod, demo1, demo2, name):
    sd = small_scene({"demo1": demo1, "demo2": demo2}[name], 16, 12)
    worst = max(against_the_oracle(flux, oracle_mod, sd, n, D, 1)[0] for n in (1, 3, 4) for D in (1, 2, 5))
    print(f"{name}: max |path_spec - oracle| = {worst:.3e}")


@pytest.mark.parametrize("case", range(8))
def test_random_scenes_of_the_sphere_and_plane_fuzz(flux, oracle_mod, demo1, case):
    """Odd cases have their plane normals normalised; even ones keep non-unit normals, NaN pixels and all (tests/test_gpu_fuzz.py)."""
    rng = np.random.default_rng(3000 + case)
    sd = random_scene(flux, demo1, rng, unit_planes=case % 2 == 1)
    # (the generator's frames reach 40 x 30: a quarter of each side keeps a case well under a second)
    sd.output_settings.image_width, sd.output_settings.image_height = max(4, sd.output_settings.image_width // 4), max(3, sd.output_settings.image_height // 4)
    n, D = int(rng.choice([2, 3, 8])), int(rng.choice([1, 3, 5, 9]))
    err, _ = against_the_oracle(flux, oracle_mod, sd, n, D, int(rng.integers(1, 1 << 30)))
    print(f"random scene {case}: {len(sd.shapes)} shapes, n {n} D {D}: max |path_spec - oracle| = {err:.3e}")


# ---- boxes: against the restatement on 12-triangle cubes --------------------------------------------------------------------------

def _box_rooms(flux):
    matte = flux.MatteData((0.7, 0.6, 0.5), (0.0, 0.0, 0.0), 0.9)
    glossy = flux.GlossyReflectiveData(0.8, (0.9, 0.8, 0.7), 20.0)
    mirror = flux.ReflectiveData(0.9, (0.9, 0.95, 1.0))
    light = flux.SphereData((0.4, 3.1, 0.3), 0.7, flux.EmissiveData((1.0, 0.9, 0.8), 4.0), False)
    ball = flux.SphereData((-1.7, 0.9, 1.1), 0.8, mirror, False)
    block = flux.BoxData((0.6, -1.9, -0.4), (2.1, -0.2, 1.3), glossy)
    crate = flux.BoxData((-2.3, -1.8, -1.6), (-0.9, -0.7, -0.3), matte)

    def scene(name, shapes, eye=(0.3, 0.4, -4.2), bg=(0.1, 0.2, 0.3)):
        return flux.SceneData(name, flux.OutputSettings(12, 9, 0.7), bg, shapes,
                              flux.CameraSettings(eye, (0.0, 0.0, 0.5), (0.0, 1.0, 0.0)), flux.CameraData(1.0, 6.0, 5.0, 0.1))
    env = flux.SphereData((0.0, 0.0, 0.0), 60.0, flux.EmissiveData((0.5, 0.6, 0.8), 1.0), True)
    return {
        # boxes seen from outside, under a sky
        "plain": scene("plain", [env, light, ball, block, crate, flux.BoxData((-6.0, -2.6, -5.0), (6.0, -2.0, 6.0), matte)]),
        # the issue's room: an inverted Matte box holding a glossy box, a Matte box, a mirror sphere and a sphere light
        "inverted": scene("inverted", [flux.BoxData((-5.0, -2.0, -5.0), (5.0, 4.0, 5.0), matte, True), block, crate, ball, light]),
        # the camera inside a mirror box (its outward normals seen from inside) that holds an emissive box and a Matte one,
        # an inverted emissive room around it for the rays the mirror's 0.9 lets through the depth limit's other end
        "nested": scene("nested", [flux.BoxData((-4.0, -2.0, -5.0), (4.0, 4.0, 5.0), mirror),
                                   flux.BoxData((0.6, 1.1, 0.2), (1.4, 1.9, 1.1), flux.EmissiveData((1.0, 0.8, 0.6), 3.0)), crate,
                                   flux.BoxData((-9.0, -9.0, -9.0), (9.0, 9.0, 9.0), flux.EmissiveData((0.2, 0.3, 0.4), 1.0), True)]),
    }


@pytest.mark.parametrize("name", ["plain", "inverted", "nested"])
def test_boxes_against_twelve_triangle_cubes(flux, oracle_mod, name):
    sd = _box_rooms(flux)[name]
    meshed = copy.deepcopy(sd)
    meshed.shapes = [s for s in sd.shapes if not isinstance(s, flux.BoxData)] + [box_as_mesh(flux, s) for s in sd.shapes if isinstance(s, flux.BoxData)]
    err, spec = against_the_oracle(flux, oracle_mod, sd, 4, 5, 3, oracle_sd=meshed)
    faces = [spec.classes[f"box face {k}"] for k in range(6)]
    print(f"box room {name}: max |path_spec - oracle on cubes| = {err:.3e}; segments per face {faces}; margins {spec.margins}")
    assert spec.min_margin() > MARGIN, spec.margins   # a scene whose margins are clear: the two may differ in nothing
    assert sum(f > 0 for f in faces) >= 5 and sum(faces) > 500   # (the scenes' own condition: the boxes are what the paths meet)


# ---- disks: the plane as a disk of radius 1e3 ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["demo1", "demo2"])
def test_a_plane_as_a_huge_disk(flux, oracle_mod, demo1, demo2, name):
    """Every hit nearer than the r = 100 environment sphere lies inside the disk, and the disk's t and hit point are the plane's
    operations in the plane's order: bit-equal."""
    plane_sd = small_scene({"demo1": demo1, "demo2": demo2}[name], 16, 12)
    sd = copy.deepcopy(plane_sd)
    planes = [i for i, s in enumerate(sd.shapes) if isinstance(s, flux.PlaneData)]
    assert planes
    for i in planes:
        p = sd.shapes[i]
        sd.shapes[i] = flux.DiskData(p.point, p.normal, 1e3, p.material)
    _, spec = against_the_oracle(flux, oracle_mod, sd, 4, 5, 2, oracle_sd=plane_sd, bit_equal=True)
    assert sum(v for k, v in spec.classes.items() if k.startswith("Disk/")) > 1000


# ---- dielectrics: two properties the spec implies -----------------------------------------------------------------------------------

def _emitter_scene(flux, extra=()):
    """Every path ends on an emitter: an inverted emissive sphere around a mirror floor, a glossy ball and a sphere light.  No
    Matte: the glossy lobe reads pixel_sets[set][index], which does not depend on the depth, and the mirror reads nothing."""
    shapes = [flux.SphereData((0.0, 0.0, 0.0), 50.0, flux.EmissiveData((0.9, 0.7, 0.5), 1.5), True),
              flux.PlaneData((0.0, -1.0, 0.0), (0.0, 1.0, 0.0), flux.ReflectiveData(0.8, (0.9, 0.9, 1.0))),
              flux.SphereData((1.6, 0.1, 1.2), 0.7, flux.GlossyReflectiveData(0.9, (0.8, 0.6, 0.4), 20.0), False),
              flux.SphereData((-2.5, 2.0, 2.0), 1.0, flux.EmissiveData((0.2, 0.9, 0.3), 4.0), False), *extra]
    return flux.SceneData("emitter", flux.OutputSettings(12, 9, 0.7), (0.0, 0.0, 0.0), shapes,
                          flux.CameraSettings((0.2, 1.5, -5.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)), flux.CameraData(1.0, 6.0, 5.0, 0.05))


def test_glass_of_index_one_changes_nothing(flux):
    """refraction_index 1 and transmit_color (1, 1, 1): F = 0 to rounding, every ray is transmitted undeviated (to rounding) with
    weight 1.  In a scene where every path ends on an emitter within the depth limit and no bounce reads a depth's hemisphere
    sample, inserting such glass only adds segments: every sample's radiance is unchanged to 1e-12."""
    white = flux.DielectricData(1.0, (1.0, 1.0, 1.0))
    glass = [flux.BoxData((-1.5, -0.6, -2.5), (0.9, 1.4, -1.2), white), flux.SphereData((-1.2, 0.2, 0.8), 0.9, white, False),
             flux.DiskData((0.4, 0.8, -0.6), (0.1, 0.3, -1.0), 1.5, white)]
    a = path_spec.PathSpec(_emitter_scene(flux), 4, 16, 5)
    b = path_spec.PathSpec(_emitter_scene(flux, glass), 4, 16, 5)
    a.frame(), b.frame()
    assert a.stats["depth_exhausted"] == b.stats["depth_exhausted"] == 0 and a.stats["misses"] == b.stats["misses"] == 0
    assert b.stats["dielectric_reflections"] == 0 and b.stats["dielectric_transmissions"] > 1000
    assert b.classes["Box/Dielectric"] > 300 and b.classes["Sphere/Dielectric"] > 100 and b.classes["Disk/Dielectric"] > 100
    assert a.stats["glossy_bounces"] > 30 and a.stats["specular_bounces"] > 500
    for k in ("glossy_bounces", "specular_bounces", "emissive_hits"):  # the same bounces and the same ends
        assert a.stats[k] == b.stats[k], k
    assert b.stats["segments"] == a.stats["segments"] + b.stats["dielectric_transmissions"]
    err = np.abs(a.sample_radiance - b.sample_radiance).max()
    print(f"index-1 glass: max per-sample |difference| = {err:.3e}")
    assert err <= SAME_SAMPLES


def test_white_furnace(flux):
    """An inverted emissive box holding glass and mirror boxes (weights 1): every sample is L or 0, and the zeros are the paths the
    depth limit ended."""
    L = 0.5
    shapes = [flux.BoxData((-6.0, -5.0, -8.0), (6.0, 5.0, 8.0), flux.EmissiveData((L, L, L), 1.0), True),
              flux.BoxData((-2.4, -1.3, -0.7), (-0.4, 0.9, 1.1), flux.ReflectiveData(1.0, (1.0, 1.0, 1.0))),
              flux.BoxData((0.3, -1.1, -0.5), (2.2, 1.2, 1.3), flux.DielectricData(1.5, (1.0, 1.0, 1.0))),
              flux.BoxData((-1.0, 1.6, 0.0), (0.8, 2.6, 1.5), flux.DielectricData(0.7, (1.0, 1.0, 1.0)))]
    sd = flux.SceneData("furnace", flux.OutputSettings(12, 9, 1.3), (0.0, 0.0, 0.0), shapes,
                        flux.CameraSettings((0.0, 0.0, -5.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)), flux.CameraData(1.0, 25.0, 25.0, 0.0))
    spec = path_spec.PathSpec(sd, 6, 6, 4)
    spec.frame()
    rad = spec.sample_radiance
    assert np.all((rad == L) | (rad == 0.0)) and np.all(rad[..., 0] == rad[..., 1]) and np.all(rad[..., 0] == rad[..., 2])
    assert int((rad[..., 0] == 0.0).sum()) == spec.stats["depth_exhausted"] > 0
    assert spec.stats["misses"] == 0 and spec.stats["emissive_hits"] + spec.stats["depth_exhausted"] == spec.stats["samples"]
    assert spec.stats["specular_bounces"] > 500 and spec.stats["dielectric_transmissions"] > 1000
    assert spec.classes["total internal reflection"] > 0 and spec.classes["reflection"] > 10


# ---- the margins' own arithmetic ----------------------------------------------------------------------------------------------------

def test_box_margin_is_rounding_level():
    o, d, _ = spec_rays(np.random.default_rng(11), 20000)
    _, _, _, _, parts = box_spec.box_hit(C0, C1, o, d)
    with np.errstate(all="ignore"):
        m = path_spec.box_margin(*parts)
    for eps in (1e-9, 1e-6, 1e-3, 1e-1):
        assert np.array_equal(m <= eps, box_spec.rounding_level(*parts, eps=eps)), eps
    assert (m <= 1e-3).sum() > 10 and (m > 1e-3).sum() > 10000


# ---- the fuzz's own scenes: margins and coverage ----------------------------------------------------------------------------------------

CLASSES = (["box face %d" % k for k in range(6)] + ["inverted box", "reflection", "transmission", "total internal reflection",
           "triangle beside a disk or box", "Sphere/Dielectric", "Plane/Dielectric", "Mesh/Dielectric"] +
           [f"{shape}/{mat}" for shape in ("Disk", "Box") for mat in ("Matte", "GlossyReflective", "Reflective", "Emissive", "Dielectric")])
DEFAULT_CHUNKS = [(False, c) for c in range(12)] + [(True, c) for c in range(4)]


@pytest.mark.parametrize("mesh,chunk", DEFAULT_CHUNKS)
def test_fuzz_chunk_takes_no_decision_at_rounding_level(flux, mesh, chunk):
    """For every scene of the default chunks the smallest margin of any decision exceeds 1e-9 -- a seed that violates this is
    changed in test_gpu_ext_fuzz.RESEEDED, nothing is excluded -- and every frame of a unit-normal scene is finite."""
    for case, (sd, n, D, seed, spec) in enumerate(ext.chunk_references(chunk, mesh)):
        assert spec.min_margin() > MARGIN, (mesh, chunk, case, spec.margins)
        assert spec.stats["samples"] == sd.output_settings.image_width * sd.output_settings.image_height * n * n
        if not ext.non_unit_normal(flux, sd):
            assert np.isfinite(spec.frame()).all(), (mesh, chunk, case)


def test_fuzz_covers_every_class():
    """Conditions on the inputs, met by the reference alone: the default chunks together hold at least 100 segments in each class."""
    total, smallest = collections.Counter(), {}
    segments = 0
    for mesh, chunk in DEFAULT_CHUNKS:
        for sd, n, D, seed, spec in ext.chunk_references(chunk, mesh):
            total.update(spec.classes)
            segments += spec.stats["segments"]
            for k, v in spec.margins.items():
                smallest[k] = min(smallest.get(k, np.inf), v)
    total["ending on a disk"] = sum(v for k, v in total.items() if k.startswith("Disk/"))
    total["on glass"] = sum(v for k, v in total.items() if k.endswith("/Dielectric"))
    print(f"extension fuzz, default chunks: {segments} segments; per class {dict(sorted(total.items()))}; smallest margins {smallest}")
    for name in CLASSES + ["ending on a disk"]:
        assert total[name] >= 100, (name, total[name])


def test_fuzz_reaches_the_forced_hit_queue(flux, demo1):
    """Among the default chunks' scenes there are enough that the split kernel runs with the forced 66-slot hit queue (unit
    normals, no glass, 64 spp or more, records and bounce list that fit), so those runs are not vacuous."""
    fits = [ext.forced_queue_fits(flux, sd, D) for chunk in range(12) for sd, n, D, seed in ext.chunk_jobs(flux, demo1, chunk, False)
            if ext.hit_queue_candidate(flux, sd, n, not ext.non_unit_normal(flux, sd))]
    with_a_box = [ext.forced_queue_fits(flux, sd, D) and any(isinstance(s, flux.BoxData) for s in sd.shapes)
                  for chunk in range(12) for sd, n, D, seed in ext.chunk_jobs(flux, demo1, chunk, False)
                  if ext.hit_queue_candidate(flux, sd, n, not ext.non_unit_normal(flux, sd))]
    print(f"forced hit queue: {len(fits)} candidate scenes, {sum(fits)} with the queue on, {sum(with_a_box)} of them with a box")
    assert sum(fits) >= 6 and sum(with_a_box) >= 3


def test_the_large_sample_count_scenes_exist():
    for k in (0, 1):
        sd, seed, spec = ext.plain_scene(k)
        assert spec.min_margin() > MARGIN and spec.stats["matte_bounces"] + spec.stats["glossy_bounces"] >= 100
