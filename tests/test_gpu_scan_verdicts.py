"""What the split kernel's scan hands its shading step without f64 geometry (render_body.inc): which side of an Emissive sphere a ray
met (sphere_facing), the environment shortcut decided in f32 first (flux_env_verdict.h), and Path::self from the lobe's own tests.
None of them may change a decision: every scene here -- emitters seen from every side, grazing and coincident ones, emitters the
scan cannot vouch for, the environment cases of tests/test_gpu_parity.py -- has the oracle's path statistics and its image to 1e-4,
and the refill and static kernels' statistics and their image to 1e-12, with the hit queue at one wave per pixel
(FLUX_SPLIT_HITQ_CAP / FLUX_SPLIT_HITQ_TAKE_AT) and with the plan's own queue.
"""
import copy

import numpy as np
import pytest

import split_checks as sc
import switches
from switches import switches as env_switches  # noqa: F401 (the fixture)
from conftest import small_scene
from split_checks import Q_LARGEST, Q_SMALLEST, REC, SLOT, SPH, TOL_ORACLE, TOL_ORDER
from test_gpu_parity import _env_cases

pytestmark = pytest.mark.gpu

QUEUES = [Q_LARGEST, Q_SMALLEST, None]
DEPTH = 5
ENV_CASES = ["convex_first", "inverted_first", "nested_environments", "camera_outside_environment", "inside_convex_matte",
             "inside_convex_glossy", "inside_convex_reflective", "beyond_the_magnitude_guard", "plane_tangent_to_the_environment",
             "sphere_across_the_environment", "spheres_touching_the_environment"]
OWN_CASES = ["camera_inside_convex_emitter", "camera_outside_convex_emitter", "inverted_emitters_from_outside", "emitter_resting_on_the_floor",
             "coincident_emitters", "coincident_emitters_swapped", "emissive_planes_both_sides", "emissive_disks_both_sides",
             "emitter_beyond_the_magnitude_guard"]


def _own_cases(flux, demo2):
    """demo2's environment, light, floor and three of its spheres, plus the emitters under test: at most 13 shapes and 12 spheres,
    so that a one-wave block still holds 86 slots."""
    base = small_scene(demo2, 24, 18)
    env = next(s for s in base.shapes if isinstance(s, flux.SphereData) and s.invert)
    light = next(s for s in base.shapes if isinstance(s, flux.SphereData) and not s.invert and isinstance(s.material, flux.EmissiveData))
    floor = next(s for s in base.shapes if isinstance(s, flux.PlaneData))
    balls = [s for s in base.shapes if isinstance(s, flux.SphereData) and s is not env and s is not light][1:4]
    matte = flux.MatteData((0.8, 0.7, 0.6), (0, 0, 0), 0.9)

    def scene(shapes, lit=True):
        sd = copy.deepcopy(base)
        sd.shapes = copy.deepcopy(([env, light] if lit else []) + balls + [floor] + shapes)
        return sd

    def emitter(center, radius, color=(0.9, 0.5, 0.3), invert=False, power=2.0):
        return flux.SphereData(tuple(center), float(radius), flux.EmissiveData(color, power), invert)

    cases = {}
    # back faces: the camera and everything it sees lie inside the scene's only emitter, so every ray meets it from inside: black
    cases["camera_inside_convex_emitter"] = scene([emitter((0.0, 0.0, 0.0), 40.0)], lit=False)
    # front faces, met by primary rays and by the bounces off the floor and the spheres around it
    cases["camera_outside_convex_emitter"] = scene([emitter((2.0, 1.5, -3.0), 1.5), flux.SphereData((-3.0, 1.0, -3.0), 1.0, matte, False)])
    # three `invert` spheres: the scan tests two of them for all lanes at once and the third lane by lane; all seen from outside: black
    cases["inverted_emitters_from_outside"] = scene([emitter((2.5, 1.5, -3.0), 1.5, invert=True), emitter((-3.0, 1.5, -3.0), 1.5, (0.2, 0.9, 0.3), True)])
    # grazing hits around the contact point, from the floor just beside it
    cases["emitter_resting_on_the_floor"] = scene([emitter((1.5, 0.75, -4.0), 0.75), emitter((-2.5, 0.5, -5.0), 0.5, (0.3, 0.5, 0.9))])
    twins = [emitter((2.0, 1.5, -3.0), 1.5), emitter((2.0, 1.5, -3.0), 1.5, (0.2, 0.9, 0.3), power=3.0)]
    cases["coincident_emitters"] = scene(twins)
    cases["coincident_emitters_swapped"] = scene(twins[::-1])
    # emitters the scan does not vouch for: one lit side towards the scene, one turned away from it
    glow = flux.EmissiveData((0.9, 0.8, 0.4), 1.5)
    planes = [flux.PlaneData((7.0, 0.0, 0.0), (-1.0, 0.0, 0.0), glow), flux.PlaneData((-7.0, 0.0, 0.0), (-1.0, 0.0, 0.0), glow)]
    cases["emissive_planes_both_sides"] = scene(planes)
    cases["emissive_disks_both_sides"] = scene([flux.DiskData(p.point, p.normal, 1e3, p.material) for p in planes])
    # a radius beyond 1e3 switches the self-skip rule off for the scene, and with it the scan's word on facing
    cases["emitter_beyond_the_magnitude_guard"] = scene([emitter((0.0, 1.0, 1530.0), 1500.0)])
    return cases


def _oracle_scene(flux, sd):
    """The oracle has no disk: one of radius 1e3 is, for these cameras, the plane it lies in (tests/test_gpu_split_hit_queue.py holds
    the two bit-equal)."""
    s = copy.deepcopy(sd)
    for k, sh in enumerate(s.shapes):
        if isinstance(sh, flux.DiskData):
            s.shapes[k] = flux.PlaneData(sh.center, sh.normal, sh.material)
    return s


_refs = {}


def _case(flux, oracle_mod, demo2, case):
    """scene, and the oracle's, the refill kernel's and the static kernel's frame and statistics: read by every queue"""
    sd = (_own_cases(flux, demo2) if case in OWN_CASES else _env_cases(flux, demo2))[case]
    return (sd,) + sc.references(_refs, case, flux, oracle_mod, sd, 16, DEPTH, 4, oracle_sd=_oracle_scene(flux, sd))


@pytest.fixture
def queue(env_switches):
    return lambda q: env_switches(**switches.queue(q))


@pytest.mark.parametrize("q", QUEUES)
@pytest.mark.parametrize("case", OWN_CASES + ENV_CASES)
def test_split_kernel_keeps_every_decision(flux, oracle_mod, demo2, queue, case, q):
    sd, want, o_stats, (refill, rs, *_), (static, ss, *_) = _case(flux, oracle_mod, demo2, case)
    queue(q)
    got, gs, plan = sc.render(flux, sd, 16, DEPTH, 4, flux.KERNEL_SPLIT)[:3]
    queue(None)
    assert plan["kernel"] == flux._lib.PLAN_SPLIT
    if q is not None and case in OWN_CASES:  # the hit queue really ran: its LDS, not the ray queue's
        n_sph = sum(isinstance(s, flux.SphereData) for s in sd.shapes)
        assert plan["lds"] == q[0] * SLOT * plan["waves_per_pixel"] + len(sd.shapes) * REC + n_sph * SPH
    assert {k: gs[k] for k in o_stats} == o_stats
    assert np.abs(got - want).max() < TOL_ORACLE
    assert gs == rs == ss, (gs, rs, ss)
    assert np.abs(got - refill).max() <= TOL_ORDER
    assert np.abs(got - static).max() <= TOL_ORDER


def test_back_faces_are_black(flux, oracle_mod, demo2, env_switches):
    """The case does what its name says, by the oracle's own frame: paths end on the emitter, and from inside it gives no light."""
    _, inside, st, _, _ = _case(flux, oracle_mod, demo2, "camera_inside_convex_emitter")
    assert st["emissive_hits"] > 0 and float(np.abs(inside).max()) == 0.0


@pytest.mark.parametrize("n,waves", [(128, 4), (96, 2)])
def test_headline_shapes(flux, demo2, n, waves):
    """demo2 at 16384 spp (K = 4, the plan's own 110-slot queue) and at 9216 spp (K = 2), 8 x 6 pixels."""
    sd = small_scene(demo2, 8, 6)
    got, gs, plan = sc.render(flux, sd, n, DEPTH, 1, flux.KERNEL_SPLIT)[:3]
    assert plan["kernel"] == flux._lib.PLAN_SPLIT and plan["waves_per_pixel"] == waves
    if n == 128:
        assert plan["lds"] == 110 * SLOT * 4 + len(sd.shapes) * REC + 12 * SPH
    refill, rs = sc.render(flux, sd, n, DEPTH, 1, flux.KERNEL_REFILL)[:2]
    static, ss = sc.render(flux, sd, n, DEPTH, 1, flux.KERNEL_STATIC)[:2]
    assert gs == rs == ss, (gs, rs, ss)
    assert np.abs(got - refill).max() <= TOL_ORDER
    assert np.abs(got - static).max() <= TOL_ORDER
