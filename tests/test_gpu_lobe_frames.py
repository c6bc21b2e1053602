"""Phase A's uniform shading step of the split kernel takes the lobe frame of a Matte hit on a record with a stored normal -- a plane, a
disk, a box face -- from the context's lobe-frame table (RenderParams::lobe_frame, filled by the device at context creation) instead of
building it per lane.  FLUX_LOBE_FRAMES=0 builds the context without the table, FLUX_SPLIT_UNIFORM_A=0 runs the general step for every
wave.  The three may not differ in a single bit: every scene here is rendered all three ways (np.array_equal, equal path statistics),
and the frame with the table has the oracle's path statistics and its image to 1e-4, and the refill and static kernels' statistics
and their image to 1e-12 -- with the plan's own queue (for demo2 at this sample count the ray queue) and with the one-wave hit queues of
tests/test_gpu_uniform_phase_a.py, so that the ray-queue and the hit-queue instantiations both run; the plan's LDS bytes say which did
(the box scene's eighteen records leave a wave 80 slots: it gets its hit queue from (66, 1), and the ray queue from (86, 22)).

24 x 18 pixels at sample root 17 (289 spp: the split kernel, one wave a pixel, a partial last pass), depth limit 5 unless the case
says otherwise.  The scenes are the smallest in which the arm can go wrong: a Matte floor alone and among demo2's spheres; a plane
whose exactly unit normal (0.6, 0.8, 0) lies on no axis; a ceiling (0, -1, 0) seen from below; the floor as a Disk; the floor as a Box
whose top and front faces are both in view (two records, two frames); a Glossy and a Reflective floor (w is the mirrored direction:
the table must not be used); a Matte plane coincident with a Glossy one in both YAML orders (the tie rule picks the record); a stored
normal that is not unit (the job is routed to STRICT, where the switch must change nothing); depth limits the first bounce meets.

The oracle knows neither disks nor boxes.  The disk of radius 1e3 is the plane it lies in for these cameras, so the oracle renders that
plane.  No set of planes is a box edge, so the case with two faces in view is held to everything but the oracle.
"""
import copy

import numpy as np
import pytest

import split_checks as sc
from conftest import small_scene
from split_checks import QUEUES, RAY_QUEUE, SLOT, TOL_ORACLE, TOL_ORDER
from switches import queue, switches as env_switches  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu

CASES = ["floor_under_the_environment", "demo2", "plane_with_an_oblique_unit_normal", "ceiling_seen_from_below", "floor_as_a_disk",
         "box_top_and_front_face", "glossy_floor", "reflective_floor", "matte_plane_before_a_coincident_glossy_one",
         "glossy_plane_before_a_coincident_matte_one", "floor_with_a_long_normal", "depth_limit_1", "depth_limit_2"]
ROUTED_TO_STRICT = ("floor_with_a_long_normal",)
PLANNED_WITH_THE_RAY_QUEUE = ("demo2",)
N, SEED = 17, 4


def _cases(flux, demo2):
    """name -> (scene, the oracle's scene or None, max_trace_depth)"""
    base = small_scene(demo2, 24, 18)
    env = next(s for s in base.shapes if isinstance(s, flux.SphereData) and s.invert)
    light = next(s for s in base.shapes if isinstance(s, flux.SphereData) and not s.invert and isinstance(s.material, flux.EmissiveData))
    floor = next(s for s in base.shapes if isinstance(s, flux.PlaneData))
    balls = [s for s in base.shapes if isinstance(s, flux.SphereData) and s is not env and s is not light]
    assert isinstance(floor.material, flux.MatteData)
    glossy = next(b.material for b in balls if isinstance(b.material, flux.GlossyReflectiveData))

    def scene(shapes, **camera):
        sd = copy.deepcopy(base)
        sd.shapes = copy.deepcopy(shapes)
        for k, v in camera.items():
            setattr(sd.camera_data if k == "lens_radius" else sd.camera_settings, k, v)
        return sd

    cases = {}

    def add(name, sd, oracle_sd="same", depth=5):
        cases[name] = (sd, sd if oracle_sd == "same" else oracle_sd, depth)

    add("floor_under_the_environment", scene([env, floor]))
    add("demo2", base)
    # a slope through the origin that rises away from the eye's right: the eye (0, 5.5, -9) is 4.4 in front of it
    add("plane_with_an_oblique_unit_normal", scene([env, light] + balls + [flux.PlaneData((0.0, 0.0, 0.0), (0.6, 0.8, 0.0), floor.material)]))
    # the eye on the floor's level looking up at a ceiling whose normal points down at it
    add("ceiling_seen_from_below", scene([env, light] + balls + [floor, flux.PlaneData((0.0, 9.0, 0.0), (0.0, -1.0, 0.0), floor.material)],
                                         eye=(0.0, 0.5, -9.0), look_at=(0.0, 9.0, 2.0)))
    add("floor_as_a_disk", scene([env, light] + balls + [flux.DiskData(floor.point, floor.normal, 1e3, floor.material)]),
        scene([env, light] + balls + [floor]))
    # a slab whose front face z = -1 stands 8 in front of the eye, below it: the bottom rows of the image see that face, the rest its top
    add("box_top_and_front_face", scene([env, light] + balls + [flux.BoxData((-1e3, -4.0, -1.0), (1e3, 0.0, 1e3), floor.material)]), None)
    add("glossy_floor", scene([env, light] + balls + [flux.PlaneData(floor.point, floor.normal, glossy)]))
    add("reflective_floor", scene([env, light] + balls + [flux.PlaneData(floor.point, floor.normal, flux.ReflectiveData(0.8, (0.9, 0.8, 0.7)))]))
    twin = flux.PlaneData(floor.point, floor.normal, glossy)
    add("matte_plane_before_a_coincident_glossy_one", scene([env, light] + balls[:4] + [floor, twin]))
    add("glossy_plane_before_a_coincident_matte_one", scene([env, light] + balls[:4] + [twin, floor]))
    add("floor_with_a_long_normal", scene([env, light] + balls + [flux.PlaneData(floor.point, (0.0, 2.0, 0.0), floor.material)]))
    add("depth_limit_1", base, depth=1)
    add("depth_limit_2", base, depth=2)
    assert sorted(cases) == sorted(CASES)
    return cases


_refs = {}


def _case(flux, oracle_mod, demo2, case):
    """scene, depth limit, and the oracle's, the refill kernel's and the static kernel's frame and statistics: read by every queue"""
    sd, oracle_sd, depth = _cases(flux, demo2)[case]
    return (sd, depth) + sc.references(_refs, case, flux, oracle_mod, sd, N, depth, SEED, oracle_sd=oracle_sd)


@pytest.fixture
def switches(env_switches):
    return lambda q=None, table=True, uniform=True: env_switches(FLUX_LOBE_FRAMES=None if table else 0,
                                                                 FLUX_SPLIT_UNIFORM_A=None if uniform else 0, **queue(q))


@pytest.mark.parametrize("q", QUEUES)
@pytest.mark.parametrize("case", CASES)
def test_table_frame_changes_no_bit(flux, oracle_mod, demo2, switches, case, q):
    switches()
    sd, depth, want, o_stats, (refill, rs, *_), (static, ss, *_) = _case(flux, oracle_mod, demo2, case)
    switches(q, table=True)
    got, gs, plan = sc.render(flux, sd, N, depth, SEED, flux.KERNEL_SPLIT)[:3]
    switches(q, table=False)
    computed, cs, plan_computed = sc.render(flux, sd, N, depth, SEED, flux.KERNEL_SPLIT)[:3]
    switches(q, table=True, uniform=False)
    general, es, plan_general = sc.render(flux, sd, N, depth, SEED, flux.KERNEL_SPLIT)[:3]
    switches()
    # which instantiation ran: the 64-entry ray queue of the plan's own choice at this sample count, or the hit queue of q[0] slots --
    # one wave a pixel, beside the scene's records (a stored normal that is not unit: STRICT has no split kernel, the refill kernel runs)
    assert plan_computed == plan and plan_general == plan
    if case in ROUTED_TO_STRICT:
        assert plan["kernel"] == flux._lib.PLAN_REFILL
    else:
        assert plan["kernel"] == flux._lib.PLAN_SPLIT and plan["waves_per_pixel"] == 1 and plan["block"] == 64
        queue = plan["lds"] - sc.scene_lds(flux, sd)
        if q is not None:
            # the planner grants q[0] slots or as many as fit (one wave a pixel: 6 of the CU's granules of 1280 B, less the scene and
            # the 96 B of the block's partial sums; an even count), and a queue of fewer than 64 + q[1] is no hit queue: the ray queue
            # runs.  The box scene's eighteen records leave 80 slots: (86, 22) gives it the ray queue, (66, 1) the hit queue.
            slots = min(q[0], (6 * 1280 - sc.scene_lds(flux, sd) - 96) // SLOT & ~1)
            assert queue == (slots * SLOT if slots >= 64 + q[1] else RAY_QUEUE)
            assert queue == q[0] * SLOT or (case, q) == ("box_top_and_front_face", (86, 22))
            assert queue == 66 * SLOT or q != (66, 1)
        else:  # (a scene of a few records leaves room for a hit queue even at this sample count; demo2's thirteen do not)
            assert queue == RAY_QUEUE or (queue % SLOT == 0 and queue >= 66 * SLOT)
            assert queue == RAY_QUEUE or case not in PLANNED_WITH_THE_RAY_QUEUE
    err_refill, err_static = (float(np.abs(got - a).max()) for a in (refill, static))
    err_oracle = None if want is None else float(np.abs(got - want).max())
    print(f"{case} {q}: |split - oracle| {err_oracle}  |split - refill| {err_refill:.3e}  |split - static| {err_static:.3e}  "
          f"bits equal without the table: {np.array_equal(got, computed)}  to the general step: {np.array_equal(got, general)}")
    assert np.array_equal(got, computed)
    assert np.array_equal(got, general)
    assert gs == cs == es, (gs, cs, es)
    assert gs == rs == ss, (gs, rs, ss)
    assert err_refill <= TOL_ORDER
    assert err_static <= TOL_ORDER
    if want is not None:
        assert {k: gs[k] for k in o_stats} == o_stats
        assert err_oracle < TOL_ORACLE


def test_the_cases_are_what_they_claim(flux, oracle_mod, demo2, switches):
    """By the kernels' own statistics: the Matte cases bounce off Matte, the Glossy and Reflective floors leave demo2's Matte bounces
    none at all, the box case sees both faces (more Matte bounces than misses past its edge would leave: some primaries hit the front
    face, whose bounces leave towards -z), and a depth limit of 1 ends every path that would bounce."""
    switches()
    st = {c: _case(flux, oracle_mod, demo2, c)[5].stats for c in CASES}
    for c in ("floor_under_the_environment", "demo2", "plane_with_an_oblique_unit_normal", "ceiling_seen_from_below", "floor_as_a_disk",
              "box_top_and_front_face", "matte_plane_before_a_coincident_glossy_one", "depth_limit_2"):
        assert st[c]["matte_bounces"] > 0, c
    for c in ("glossy_floor", "reflective_floor"):
        assert st[c]["matte_bounces"] == 0, c
    # the tie rule: the first of the coincident planes in YAML order is the one that is hit
    assert st["glossy_plane_before_a_coincident_matte_one"]["matte_bounces"] == 0
    assert st["depth_limit_1"]["segments"] == st["depth_limit_1"]["samples"] and st["depth_limit_1"]["depth_exhausted"] > 0
    # both faces of the box: its primaries' hits are all Matte, and a frame of the top face alone (the same slab, its front face
    # pushed out of view) has a different count
    sd, depth = _case(flux, oracle_mod, demo2, "box_top_and_front_face")[:2]
    top_only = copy.deepcopy(sd)
    box = next(s for s in top_only.shapes if isinstance(s, flux.BoxData))
    box.corner0 = (box.corner0[0], box.corner0[1], -1e3)
    other = sc.render(flux, top_only, N, depth, SEED, flux.KERNEL_STATIC).stats
    assert other["matte_bounces"] != st["box_top_and_front_face"]["matte_bounces"]
