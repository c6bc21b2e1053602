"""Phase A of the split kernel shades a wave whose primaries all hit one shape -- or all miss -- from that shape's record as a
scalar (render_body.inc shade_primary_hits); FLUX_SPLIT_UNIFORM_A=0 runs the general, per-lane step for every wave.  The two may not
differ in a single bit: every scene here is rendered both ways (np.array_equal, equal path statistics), and the frame with the
uniform step has the oracle's path statistics and its image to 1e-4, and the refill and static kernels' statistics and their image
to 1e-12 -- with the plan's own hit queue and with one-wave queues (FLUX_SPLIT_HITQ_CAP / FLUX_SPLIT_HITQ_TAKE_AT).

The scenes: waves that are all uniform (a floor under the environment; a camera whose whole view is one sphere, so Path::self is
set; an emissive plane from either side; nothing but misses), waves that pass the vote beside waves that fail it (demo2's defocused
sphere edges), the floor as a Disk and as a Box (other instantiations of the kernel), a stored normal that is not unit (at this depth the job
is routed to the STRICT arithmetic and the switch must change nothing there either), coincident shapes (the tie rule hands every lane the same record), slices that end in a
partial pass (289 spp: the lanes past the end have no vote), and depth limits the first bounce meets.
"""
import copy

import numpy as np
import pytest

import split_checks as sc
from conftest import small_scene
from split_checks import QUEUES, TOL_ORACLE, TOL_ORDER
from switches import queue, switches as env_switches  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu

SEED = 4
CASES = ["floor_under_the_environment", "demo2", "close_to_a_glossy_sphere", "close_to_a_reflective_sphere", "close_to_a_matte_sphere",
         "emissive_plane_lit_side", "emissive_plane_from_behind", "floor_as_a_disk", "floor_as_a_box", "floor_with_a_long_normal",
         "coincident_planes", "plane_coincident_with_a_disk", "outside_the_environment_looking_away", "partial_last_pass",
         "depth_limit_1", "depth_limit_2"]


def _cases(flux, demo2):
    """name -> (scene, the oracle's scene, sample_root, max_trace_depth)"""
    base = small_scene(demo2, 24, 18)
    env = next(s for s in base.shapes if isinstance(s, flux.SphereData) and s.invert)
    light = next(s for s in base.shapes if isinstance(s, flux.SphereData) and not s.invert and isinstance(s.material, flux.EmissiveData))
    floor = next(s for s in base.shapes if isinstance(s, flux.PlaneData))
    balls = [s for s in base.shapes if isinstance(s, flux.SphereData) and s is not env and s is not light]

    def scene(shapes, **camera):
        sd = copy.deepcopy(base)
        sd.shapes = copy.deepcopy(shapes)
        for k, v in camera.items():
            setattr(sd.camera_data if k == "lens_radius" else sd.camera_settings, k, v)
        return sd

    def with_floor(new_floor, oracle_floor=None):
        sd = scene([env, light] + balls + [new_floor])
        return sd, (sd if oracle_floor is None else scene([env, light] + balls + [oracle_floor]))

    def close_to(material):
        # the eye 2.3 from the centre of a unit sphere: it fills the 22-degree half-angle of view, so every primary hits it
        ball = copy.deepcopy(balls[0])
        ball.material = material
        return scene([env, light, ball] + balls[1:] + [floor], eye=(-2.0, 1.6, -6.2), look_at=ball.center, lens_radius=0.0)

    cases = {}

    def add(name, sd, oracle_sd=None, n=16, depth=5):
        cases[name] = (sd, sd if oracle_sd is None else oracle_sd, n, depth)

    add("floor_under_the_environment", scene([env, floor]))
    add("demo2", base)
    add("close_to_a_glossy_sphere", close_to(balls[0].material))
    add("close_to_a_reflective_sphere", close_to(flux.ReflectiveData(0.8, (0.9, 0.8, 0.7))))
    add("close_to_a_matte_sphere", close_to(flux.MatteData((0.8, 0.7, 0.6), (0, 0, 0), 0.9)))
    glow = flux.EmissiveData((0.9, 0.8, 0.4), 1.5)
    add("emissive_plane_lit_side", scene([env] + balls[:3] + [floor, flux.PlaneData((0.0, 0.0, 20.0), (0.0, 0.0, -1.0), glow)]))
    add("emissive_plane_from_behind", scene([env] + balls[:3] + [floor, flux.PlaneData((0.0, 0.0, 20.0), (0.0, 0.0, 1.0), glow)]))
    # the oracle has neither shape: for these cameras a disk of radius 1e3 is the plane it lies in, and so is the top face of a box
    # that reaches as far (no ray that starts above the floor meets another face)
    add("floor_as_a_disk", *with_floor(flux.DiskData(floor.point, floor.normal, 1e3, floor.material), floor))
    add("floor_as_a_box", *with_floor(flux.BoxData((-1e3, -1.0, -1e3), (1e3, 0.0, 1e3), floor.material), floor))
    add("floor_with_a_long_normal", *with_floor(flux.PlaneData(floor.point, (0.0, 2.0, 0.0), floor.material)))
    other = flux.MatteData((0.2, 0.7, 0.3), (0, 0, 0), 0.8)
    add("coincident_planes", scene([env, light] + balls[:4] + [floor, flux.PlaneData(floor.point, floor.normal, other)]))
    twin = [env, light] + balls[:4] + [flux.DiskData(floor.point, floor.normal, 1e3, other), floor]
    add("plane_coincident_with_a_disk", scene(twin), scene(twin[:-2] + [flux.PlaneData(floor.point, floor.normal, other), floor]))
    away = scene([env, light] + balls, eye=(0.0, 5.5, -300.0), look_at=(0.0, 5.5, -400.0))
    away.background = (0.2, 0.3, 0.4)
    add("outside_the_environment_looking_away", away)
    add("partial_last_pass", base, n=17)
    add("depth_limit_1", base, depth=1)
    add("depth_limit_2", base, depth=2)
    return cases


_refs = {}


def _case(flux, oracle_mod, demo2, case):
    """scene, sample root, depth limit, and the oracle's, the refill kernel's and the static kernel's frame and statistics: read by
    every queue"""
    sd, oracle_sd, n, depth = _cases(flux, demo2)[case]
    return (sd, n, depth) + sc.references(_refs, case, flux, oracle_mod, sd, n, depth, SEED, oracle_sd=oracle_sd)


@pytest.fixture
def switches(env_switches):
    return lambda q, uniform: env_switches(FLUX_SPLIT_UNIFORM_A=None if uniform else 0, **queue(q))


@pytest.mark.parametrize("q", QUEUES)
@pytest.mark.parametrize("case", CASES)
def test_uniform_step_changes_no_bit(flux, oracle_mod, demo2, switches, case, q):
    sd, n, depth, want, o_stats, (refill, rs, *_), (static, ss, *_) = _case(flux, oracle_mod, demo2, case)
    switches(q, True)
    got, gs, plan = sc.render(flux, sd, n, depth, SEED, flux.KERNEL_SPLIT)[:3]
    switches(q, False)
    general, es, plan_general = sc.render(flux, sd, n, depth, SEED, flux.KERNEL_SPLIT)[:3]
    switches(None, True)
    # (a stored normal that is not unit routes the job to the STRICT arithmetic, which has no split kernel: the refill kernel runs,
    # with or without the switch)
    assert plan["kernel"] == (flux._lib.PLAN_REFILL if case == "floor_with_a_long_normal" else flux._lib.PLAN_SPLIT)
    assert plan_general == plan
    err_oracle, err_refill, err_static = (float(np.abs(got - a).max()) for a in (want, refill, static))
    print(f"{case} {q}: |split - oracle| {err_oracle:.3e}  |split - refill| {err_refill:.3e}  |split - static| {err_static:.3e}  "
          f"bits equal to the general step: {np.array_equal(got, general)}")
    assert gs == rs == ss, (gs, rs, ss)
    assert err_refill <= TOL_ORDER
    assert err_static <= TOL_ORDER
    assert {k: gs[k] for k in o_stats} == o_stats
    assert err_oracle < TOL_ORACLE
    assert np.array_equal(got, general)
    assert gs == es, (gs, es)


def test_the_cases_are_what_they_claim(flux, oracle_mod, demo2, env_switches):
    """By the oracle's own statistics: the all-miss scene only misses, the view from behind the emissive plane sees less light than
    the one from its lit side, and a depth limit of 1 ends every path that would bounce."""
    st = {c: _case(flux, oracle_mod, demo2, c)[4] for c in ("outside_the_environment_looking_away", "depth_limit_1")}
    away = st["outside_the_environment_looking_away"]
    assert away["misses"] == away["samples"] == away["segments"] > 0
    assert st["depth_limit_1"]["segments"] == st["depth_limit_1"]["samples"] and st["depth_limit_1"]["depth_exhausted"] > 0
    lit = _case(flux, oracle_mod, demo2, "emissive_plane_lit_side")[3]
    behind = _case(flux, oracle_mod, demo2, "emissive_plane_from_behind")[3]
    assert float(lit.sum()) > float(behind.sum())
