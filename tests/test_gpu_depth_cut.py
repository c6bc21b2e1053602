"""The split kernel's depth cut (launch_plan.cpp split_cut_depth): phase B ends a path whose hit at the depth limit would bounce --
its child ends with L = 0 untraced -- instead of parking the hit (the hit queue) or holding the dead path through one more pass (the
ray queue).  FLUX_SPLIT_DEPTH_CUT=0 turns it off.  Nothing a frame is made of changes: every scene here is rendered both ways with
equal path statistics -- the cut counts what the skipped bounce and the skipped pass counted -- and frames within 1e-12 (which lane
takes which parked hit shifts, so the order of a pixel's sum does), and the frame with the cut has the refill and the static kernels'
statistics and their image to 1e-12, the oracle's statistics and its image to 1e-4, is the same bit for bit when rendered again, and
row by row when rendered as a sub-range -- with the plan's own queue (at 256 spp the ray queue) and with one-wave hit queues
(FLUX_SPLIT_HITQ_CAP / FLUX_SPLIT_HITQ_TAKE_AT).

The scenes: demo2 at depth limits 1 (no phase-B hit reaches the limit), 2 (every candidate for the queue is at the limit: it stays
empty), 3 and 5; a camera whose whole view is a Reflective sphere (the specular counter) and a Matte one; the floor as a Disk and as
a Box (the instantiations outside TYP; the Box scene's 17 records get a throughput table at depth 3 and none at depth 5, where the
hit queue must keep parking); a glass sphere beside the balls (a Dielectric scene keeps the ray queue, whose cut follows the
bounce); 289 spp (a partial last pass); and a 32x24 job at 64 spp in the ray-queue loop.  A floor of colour 1e200 makes throughputs
that are not finite: the context must refuse the hit queue's cut, so the switch changes no bit.  CPU side: tests/test_depth_cut.py."""
import copy

import numpy as np
import pytest

import split_checks as sc
from conftest import small_scene
from split_checks import QUEUES, TOL_ORACLE, TOL_ORDER
from switches import queue, switches as env_switches  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu

CASES = ["demo2_depth_1", "demo2_depth_2", "demo2_depth_3", "demo2", "close_to_a_reflective_sphere", "reflective_sphere_depth_2",
         "close_to_a_matte_sphere", "floor_as_a_disk", "floor_as_a_box_depth_3", "floor_as_a_box", "glass_beside_the_balls",
         "partial_last_pass"]
NO_ORACLE = ("glass_beside_the_balls",)  # the oracle has no Dielectric: the static and refill kernels stand in
SEED = 4


def _cases(flux, demo2):
    """name -> (scene, the oracle's scene, sample_root, max_trace_depth)"""
    base = small_scene(demo2, 24, 18)
    env = next(s for s in base.shapes if isinstance(s, flux.SphereData) and s.invert)
    light = next(s for s in base.shapes if isinstance(s, flux.SphereData) and not s.invert and isinstance(s.material, flux.EmissiveData))
    floor = next(s for s in base.shapes if isinstance(s, flux.PlaneData))
    balls = [s for s in base.shapes if isinstance(s, flux.SphereData) and s is not env and s is not light]

    def scene(shapes, like=base, **camera):
        sd = copy.deepcopy(like)
        sd.shapes = copy.deepcopy(shapes)
        for k, v in camera.items():
            setattr(sd.camera_data if k == "lens_radius" else sd.camera_settings, k, v)
        return sd

    def with_floor(new_floor):
        # the oracle has neither shape: for these cameras a disk of radius 1e3 is the plane it lies in, and so is the top face of a
        # box that reaches as far (no ray that starts above the floor meets another face)
        return scene([env, light] + balls + [new_floor]), scene([env, light] + balls + [floor])

    def close_to(material):
        # the eye 2.3 from the centre of a unit sphere: it fills the 22-degree half-angle of view, so every primary hits it
        ball = copy.deepcopy(balls[0])
        ball.material = material
        return scene([env, light, ball] + balls[1:] + [floor], eye=(-2.0, 1.6, -6.2), look_at=ball.center, lens_radius=0.0)

    cases = {}

    def add(name, sd, oracle_sd=None, n=16, depth=5):
        cases[name] = (sd, sd if oracle_sd is None else oracle_sd, n, depth)

    for depth in (1, 2, 3):
        add(f"demo2_depth_{depth}", base, depth=depth)
    add("demo2", base)
    mirror = close_to(flux.ReflectiveData(0.8, (0.9, 0.8, 0.7)))
    add("close_to_a_reflective_sphere", mirror)
    add("reflective_sphere_depth_2", mirror, depth=2)
    add("close_to_a_matte_sphere", close_to(flux.MatteData((0.8, 0.7, 0.6), (0, 0, 0), 0.9)))
    add("floor_as_a_disk", *with_floor(flux.DiskData(floor.point, floor.normal, 1e3, floor.material)))
    box = with_floor(flux.BoxData((-1e3, -1.0, -1e3), (1e3, 0.0, 1e3), floor.material))
    add("floor_as_a_box_depth_3", *box, depth=3)
    add("floor_as_a_box", *box)
    glass = copy.deepcopy(balls)
    glass[1].material = flux.DielectricData(1.5, (0.9, 1.0, 0.95))
    add("glass_beside_the_balls", scene([env, light] + glass + [floor]))
    add("partial_last_pass", base, n=17)
    add("ray_queue_job", scene(base.shapes, like=small_scene(demo2, 32, 24)), n=8)
    bright = copy.deepcopy(floor)
    bright.material = flux.MatteData((1e200, 1e200, 1e200), (0, 0, 0), 1.0)
    add("floor_of_colour_1e200", scene([env, light] + balls + [bright]))
    return cases


@pytest.fixture
def switches(env_switches):
    return lambda q, cut: env_switches(FLUX_SPLIT_DEPTH_CUT=None if cut else 0, **queue(q))


_refs = {}


def _case(flux, oracle_mod, demo2, case):
    """scene, sample root, depth limit, and the oracle's, the refill kernel's and the static kernel's frame and statistics: read by
    every queue"""
    sd, oracle_sd, n, depth = _cases(flux, demo2)[case]
    return (sd, n, depth) + sc.references(_refs, case, flux, oracle_mod, sd, n, depth, SEED,
                                          oracle_sd=None if case in NO_ORACLE else oracle_sd)


def _check(flux, oracle_mod, demo2, switches, case, q):
    sd, n, depth, want, o_stats, (refill, rs, *_), (static, ss, *_) = _case(flux, oracle_mod, demo2, case)
    first, last = 5, 11
    switches(q, True)
    # the frame once more and a sub-range of its rows from the same context
    with flux.Renderer(sd, flux.JobConfiguration(n, depth, 50), seed=SEED) as r:
        got, gs = sc.with_stats(flux, r, flux.KERNEL_SPLIT)
        plan, again, rows = r.launch_plan(), r.render_frame(), r.render_rows(first, last)
    switches(q, False)
    uncut, us, plan_uncut = sc.render(flux, sd, n, depth, SEED, flux.KERNEL_SPLIT)[:3]
    switches(None, True)
    assert plan["kernel"] == flux._lib.PLAN_SPLIT
    assert plan_uncut == plan
    err_uncut, err_refill, err_static = (float(np.abs(got - a).max()) for a in (uncut, refill, static))
    err_oracle = float(np.abs(got - want).max()) if want is not None else float("nan")
    print(f"{case} {q}: |cut - uncut| {err_uncut:.3e}  |cut - refill| {err_refill:.3e}  |cut - static| {err_static:.3e}  "
          f"|cut - oracle| {err_oracle:.3e}  depth_exhausted {gs['depth_exhausted']}")
    assert gs == us, (gs, us)
    assert gs == rs == ss, (gs, rs, ss)
    assert err_uncut <= TOL_ORDER
    assert err_refill <= TOL_ORDER
    assert err_static <= TOL_ORDER
    if want is not None:
        assert {k: gs[k] for k in o_stats} == o_stats
        assert err_oracle < TOL_ORACLE
    else:
        assert ss["dielectric_reflections"] > 0 and ss["dielectric_transmissions"] > 0 and ss["depth_exhausted"] > 0
    assert np.array_equal(got, again)
    assert np.array_equal(rows, got[first:last + 1])


@pytest.mark.parametrize("q", QUEUES)
@pytest.mark.parametrize("case", CASES)
def test_depth_cut_changes_no_result(flux, oracle_mod, demo2, switches, case, q):
    _check(flux, oracle_mod, demo2, switches, case, q)


def test_depth_cut_in_the_ray_queue_loop(flux, oracle_mod, demo2, switches):
    """32x24 at 64 spp, the plan's own queue: one wave a pixel, no hit queue."""
    _check(flux, oracle_mod, demo2, switches, "ray_queue_job", None)


def test_the_cut_has_paths_to_end(flux, oracle_mod, demo2, env_switches):
    """By the oracle's own statistics: at depth 5 demo2 has paths that the depth limit ends, and at depth 2 those are exactly the hits
    that bounce at depth 2 -- every bounce of the depth-2 run but the primaries', which the depth-1 run counts as depth_exhausted."""
    st = {d: _case(flux, oracle_mod, demo2, "demo2" if d == 5 else f"demo2_depth_{d}")[4] for d in (1, 2, 5)}
    bounces = lambda s: s["matte_bounces"] + s["glossy_bounces"] + s["specular_bounces"]  # noqa: E731
    assert st[5]["depth_exhausted"] > 0
    assert st[1]["depth_exhausted"] == bounces(st[1]) > 0
    assert st[2]["depth_exhausted"] == bounces(st[2]) - bounces(st[1]) > 0
    mirror = _case(flux, oracle_mod, demo2, "reflective_sphere_depth_2")[4]
    assert mirror["specular_bounces"] > 0 and mirror["depth_exhausted"] > 0


@pytest.mark.parametrize("q", QUEUES[1:])
def test_throughputs_that_are_not_finite_refuse_the_cut(flux, demo2, switches, q):
    """A floor of Matte colour 1e200: the throughput of two floor bounces is infinite, so ending a path with 0 * (the throughput before
    its last bounce) is not what the later pass adds.  The context refuses the hit queue's cut -- seen here as bit equality: the
    switch changes nothing -- and the pixels that are finite are the refill kernel's."""
    sd, _, n, depth = _cases(flux, demo2)["floor_of_colour_1e200"]
    switches(q, True)
    got, gs, plan = sc.render(flux, sd, n, depth, SEED, flux.KERNEL_SPLIT)[:3]
    switches(q, False)
    uncut, us = sc.render(flux, sd, n, depth, SEED, flux.KERNEL_SPLIT)[:2]
    switches(None, True)
    refill, rs = sc.render(flux, sd, n, depth, SEED, flux.KERNEL_REFILL)[:2]
    assert plan["kernel"] == flux._lib.PLAN_SPLIT
    assert not np.isfinite(refill).all() and np.isfinite(refill).any()
    assert np.array_equal(got, uncut, equal_nan=True)
    assert np.array_equal(got.view(np.uint64), uncut.view(np.uint64))
    assert gs == us == rs
    assert np.array_equal(np.isfinite(got), np.isfinite(refill))
