"""The split kernel's hit queue over the kinds of hit it parks (flux_plan.h; render_body.inc render_split_kernel): the pool is an array
of 17-dword slots, and a batch bounces Matte and Glossy hits, on stored normals and on spheres, side by side.  (Two entry classes --
a 36-byte entry for a Matte hit on a stored normal -- were built on this layout, measured slower and not kept: DESIGN.md section 4; the
scenes below are the ones that told the classes apart.)  Each sample's arithmetic is the immediate bounce's, so against the static
kernel the images are equal to the summation order (1e-12, tests/test_gpu_split_hit_queue.py) and the path statistics equal the
oracle's exactly (the oracle knows no Disk, Box or Dielectric: here the three shipped scenes that have one are held against the
static kernel's statistics only; the independent reference for such scenes is tests/path_spec.py, against which
tests/test_gpu_ext_fuzz.py holds every kernel, the forced hit queue included, on random scenes); decisions are counts, so frames are
bit-reproducible and independent of how they are sharded.

Scenes (16 x 12 pixels at 256 spp, the split kernel's floor, and at 1024 spp: one wave a pixel, whose LDS share holds the hit queue
only under the overrides below; 8 x 6 pixels at 16384 spp: four waves a pixel and the plan's own pool of 110 slots or more):
  demo2          Matte hits on the plane, Glossy ones on spheres
  matte_plane    two Matte planes and emitters: every parked hit is a Matte one on a stored normal
  glossy         glossy spheres over an Emissive floor: none is
  matte_sphere   a Matte sphere on the Matte plane: the same material on a stored normal and on a sphere's
  disk_light     not TYP; Matte on a disk
  box_room       not TYP; Matte and Glossy on box faces
  glass          not TYP; a scene with a dielectric keeps the ray queue
Queues: the plan's own (the ray queue for a one-wave block where fewer than 96 slots fit); the smallest pool the plan accepts (66
slots, so H = 2: the pool fills and the room test refuses phase A); H = 1 (one-hit batches).  Depth limits 1, 2 and 5: at 2 every
parked hit is at the limit.
"""
import copy
import os

import numpy as np
import pytest

import split_checks as sc
import switches
from switches import switches as env_switches  # noqa: F401 (the fixture)
from conftest import SCENES, small_scene
from split_checks import RAY_QUEUE, SLOT, TOL_ORDER

pytestmark = pytest.mark.gpu

W, H, SEED = 16, 12, 1
SCENE_NAMES = ["demo2", "matte_plane", "glossy", "matte_sphere", "disk_light", "box_room", "glass"]
NOT_IN_THE_ORACLE = ("disk_light", "box_room", "glass")
# FLUX_SPLIT_HITQ_CAP, FLUX_SPLIT_HITQ_TAKE_AT
QUEUES = {"plan": (None, None), "smallest": (66, 2), "take1": (None, 1)}


@pytest.fixture(scope="module")
def scenes(flux, demo2):
    return _scenes(flux, demo2, W, H)


@pytest.fixture(scope="module")
def scenes_8x6(flux, demo2):
    return _scenes(flux, demo2, 8, 6)


def _scenes(flux, demo2, W, H):
    env, light = demo2.shapes[0], demo2.shapes[1]
    spheres = [s for s in demo2.shapes[2:] if isinstance(s, flux.SphereData)]
    plane = next(s for s in demo2.shapes if isinstance(s, flux.PlaneData))
    assert isinstance(env.material, flux.EmissiveData) and isinstance(light.material, flux.EmissiveData)
    assert isinstance(plane.material, flux.MatteData) and len(spheres) == 10

    def with_shapes(shapes):
        sd = copy.deepcopy(small_scene(demo2, W, H))
        sd.shapes = copy.deepcopy(shapes)
        return sd

    # (a Matte wall across the floor, so that bounces off the one land on the other: hits for phase B to park)
    wall = flux.PlaneData((0.0, 0.0, 6.0), (0.0, 0.0, -1.0), plane.material)
    out = {"demo2": small_scene(demo2, W, H), "matte_plane": with_shapes([env, light, plane, wall])}
    floor = copy.deepcopy(plane)
    floor.material = light.material
    out["glossy"] = with_shapes([env, light] + spheres + [floor])
    ball = copy.deepcopy(spheres[4])
    ball.material = plane.material
    out["matte_sphere"] = with_shapes([env, light, ball, plane])
    for name in ("disk_light", "box_room", "glass"):
        out[name] = small_scene(flux.load_scene(os.path.join(SCENES, name + ".yml")), W, H)
    return out


def _has_dielectric(flux, sd):
    return any(isinstance(s.material, flux.DielectricData) for s in sd.shapes)


@pytest.fixture
def queue(env_switches):
    return lambda name: env_switches(**switches.queue(QUEUES[name]))


_refs = {}   # per scene, sample root and depth limit: the oracle's statistics and the static kernel's run, under the plan's own queue


def _cases():
    for name in SCENE_NAMES:
        for n in (16, 32):
            for q in QUEUES:
                for depth in (1, 2, 5):
                    yield name, n, q, depth
        for depth in (2, 5):
            yield name, 128, "plan", depth


@pytest.mark.parametrize("name,n,q,depth", list(_cases()))
def test_split_equals_static_and_the_oracles_statistics(flux, oracle_mod, scenes, scenes_8x6, queue, name, n, q, depth):
    sd = (scenes_8x6 if n == 128 else scenes)[name]
    _, ost, (want, ws, *_) = sc.references(_refs, (name, n, depth), flux, oracle_mod, sd, n, depth, SEED, kernels=("STATIC",),
                                           oracle_sd=None if name in NOT_IN_THE_ORACLE else sc.SAME)
    queue(q)
    got, gs, plan = sc.render(flux, sd, n, depth, SEED, flux.KERNEL_SPLIT)[:3]
    queue("plan")
    assert plan["kernel"] == flux._lib.PLAN_SPLIT and plan["waves_per_pixel"] == (4 if n == 128 else 1)
    queues = (plan["lds"] - sc.scene_lds(flux, sd)) // plan["waves_per_pixel"]
    if _has_dielectric(flux, sd):
        assert queues == RAY_QUEUE
    elif q == "smallest":
        assert queues == 66 * SLOT
    elif q == "take1" or n == 128:  # every slot that fits: 110 or more a wave of a four-wave block for these scenes' records
        assert queues % SLOT == 0 and queues >= (110 if n == 128 else 65) * SLOT
    assert gs == ws
    if name not in NOT_IN_THE_ORACLE:
        assert {k: ws[k] for k in ost} == ost and {k: gs[k] for k in ost} == ost
    if depth > 1 and name != "glossy":
        assert gs["matte_bounces"] > 0
    assert np.abs(got - want).max() <= TOL_ORDER


@pytest.mark.parametrize("n,q", [(32, "smallest"), (32, "take1"), (128, "plan")])
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_repeated_frames_and_shards_are_bit_equal(flux, scenes, scenes_8x6, queue, name, n, q):
    sd = (scenes_8x6 if n == 128 else scenes)[name]
    cfg = flux.JobConfiguration(n, 5, 50)
    queue(q)
    with flux.Renderer(sd, cfg, seed=2) as r:
        r.set_kernel(flux.KERNEL_SPLIT)
        a = r.render_frame()
        assert np.array_equal(a, r.render_frame())
        assert np.array_equal(r.render_rows(1, 4), a[1:5])
    for mode in (flux.SHARD_SETS, flux.SHARD_ROWS):
        with flux.MultiRenderer(sd, cfg, seed=2, devices=[0, 0, 0], shard=mode | flux._lib.SHARD_LOOPBACK) as m:
            assert np.array_equal(m.render_frame(), a), mode
