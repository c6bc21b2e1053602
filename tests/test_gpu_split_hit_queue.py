"""The split kernel's hit queue (render_body.inc; kHitQBytesPerSlot in flux_plan.h): phase B parks its continuing hits in LDS and bounces them in
batches.  Each sample's arithmetic is the immediate bounce's, so against the refill and static kernels the path statistics are
identical and the images equal to the summation order (1e-12); decisions are counts, so frames are bit-reproducible and independent
of how they are sharded.  FLUX_SPLIT_HITQ_CAP / FLUX_SPLIT_HITQ_TAKE_AT (read by the launch plan) reach the small queues and the
one-hit batches a default plan does not choose.
"""
import copy

import numpy as np
import pytest

import split_checks as sc
import switches
from switches import switches as env_switches  # noqa: F401 (the fixture)
from conftest import small_scene
from split_checks import Q_LARGEST, Q_SMALLEST, RAY_QUEUE, SLOT, TOL_ORACLE, TOL_ORDER

pytestmark = pytest.mark.gpu

DEPTH, SEED = 5, 1
# (C, H): None = the plan's own choice; the smallest queue (64 + 2: a pass's 64 continuations and room to spare), one-hit batches;
# a middling one; the largest a one-wave block holds for demo2 (86 slots)
QUEUES = [None, Q_SMALLEST, (80, 16), Q_LARGEST]


def _plane_to_disk(flux, sd, radius=1e3):
    s = copy.deepcopy(sd)
    for i, sh in enumerate(s.shapes):
        if isinstance(sh, flux.PlaneData):
            s.shapes[i] = flux.DiskData(sh.point, sh.normal, radius, sh.material)
    return s


@pytest.fixture
def queue(env_switches):
    return lambda q: env_switches(**switches.queue(q))


def _scenes(flux, demo1, demo2):
    return {"demo1": small_scene(demo1, 40, 30), "demo2": small_scene(demo2, 40, 30),
            "disk": _plane_to_disk(flux, small_scene(demo2, 40, 30))}


def test_headline_plan_holds_110_slots(flux, demo2):
    """demo2 at 16384 spp (K = 4): 25 LDS granules per block at 5 waves/SIMD, less the scene copy and `part`: 110 slots a wave."""
    sd = small_scene(demo2, 8, 6)
    with flux.Renderer(sd, flux.JobConfiguration(128, 5, 50), seed=1) as r:
        r.set_kernel(flux.KERNEL_DEFAULT)
        plan = r.launch_plan()
    assert plan["kernel"] == flux._lib.PLAN_SPLIT and plan["waves_per_pixel"] == 4
    assert plan["lds"] == 110 * SLOT * 4 + sc.scene_lds(flux, sd)
    assert plan["lds"] + 96 <= 25 * 1280


@pytest.mark.parametrize("q", QUEUES)
@pytest.mark.parametrize("n", [2, 4, 8, 16, 32])
@pytest.mark.parametrize("scene", ["demo1", "demo2", "disk"])
def test_split_equals_refill_and_static(flux, demo1, demo2, queue, scene, n, q):
    sd = _scenes(flux, demo1, demo2)[scene]
    want, ws = sc.render(flux, sd, n, DEPTH, SEED, flux.KERNEL_REFILL)[:2]
    stat, ss = sc.render(flux, sd, n, DEPTH, SEED, flux.KERNEL_STATIC)[:2]
    queue(q)
    got, gs, plan = sc.render(flux, sd, n, DEPTH, SEED, flux.KERNEL_SPLIT)[:3]
    if n * n >= 64:
        assert plan["kernel"] == flux._lib.PLAN_SPLIT
        if q is not None:  # the override reaches the kernel: the hit queue's LDS, not the ray queue's
            assert plan["lds"] == q[0] * SLOT * plan["waves_per_pixel"] + sc.scene_lds(flux, sd)
    assert gs == ws == ss, (gs, ws, ss)
    assert np.abs(got - want).max() <= TOL_ORDER
    assert np.abs(got - stat).max() <= TOL_ORDER


@pytest.mark.parametrize("q", [Q_SMALLEST, Q_LARGEST])
@pytest.mark.parametrize("scene,n", [("demo1", 16), ("demo2", 16), ("demo2", 32)])
def test_split_against_the_oracle(flux, oracle_mod, demo1, demo2, queue, scene, n, q):
    sd = _scenes(flux, demo1, demo2)[scene]
    want_o = oracle_mod.Oracle(sd, flux.JobConfiguration(n, 5, 50), seed=1)
    want = want_o.render_frame(threads=8)
    queue(q)
    got, gs = sc.render(flux, sd, n, DEPTH, SEED, flux.KERNEL_SPLIT)[:2]
    assert np.abs(got - want).max() < TOL_ORACLE
    o_stats = want_o.stats()
    assert {k: gs[k] for k in o_stats} == o_stats


@pytest.mark.parametrize("q", [None, Q_SMALLEST, Q_LARGEST])
def test_determinism_and_row_bands(flux, demo2, queue, q):
    sd = small_scene(demo2, 40, 30)
    queue(q)
    with flux.Renderer(sd, flux.JobConfiguration(32, 5, 50), seed=2) as r:
        r.set_kernel(flux.KERNEL_SPLIT)
        a = r.render_frame()
        assert np.array_equal(a, r.render_frame())
        for lo, hi in ((0, 0), (3, 9), (10, 29)):
            assert np.array_equal(r.render_rows(lo, hi), a[lo:hi + 1])


@pytest.mark.parametrize("q", [None, Q_SMALLEST, Q_LARGEST])
@pytest.mark.parametrize("n", [16, 32])
def test_plane_and_disk_bit_equal(flux, demo1, demo2, queue, n, q):
    queue(q)
    for name in ("demo1", "demo2"):
        plane = small_scene(demo1 if name == "demo1" else demo2, 40, 30)
        a, sa, pa = sc.render(flux, plane, n, DEPTH, SEED, flux.KERNEL_SPLIT)[:3]
        b, sb, pb = sc.render(flux, _plane_to_disk(flux, plane), n, DEPTH, SEED, flux.KERNEL_SPLIT)[:3]
        assert pa["lds"] == pb["lds"]
        assert sa == sb and np.array_equal(a, b), (name, n)


def test_records_that_leave_no_room_fall_back(flux, demo2):
    """96 extra planes far below the floor: 13 KiB of records leave a 4-wave block (16384 spp) fewer than 96 slots a wave, so the
    kernel keeps the ray queue and bounces at once -- with the same statistics and image as the refill kernel."""
    base = small_scene(demo2, 4, 3)
    sd = copy.deepcopy(base)
    for k in range(96):
        sd.shapes.append(flux.PlaneData((0.0, -1e4 - k, 0.0), (0.0, 1.0, 0.0), base.shapes[-1].material))
    lds = sc.scene_lds(flux, sd)
    assert lds <= 16384
    got, gs, plan = sc.render(flux, sd, 128, DEPTH, SEED, flux.KERNEL_SPLIT)[:3]
    assert plan["kernel"] == flux._lib.PLAN_SPLIT and plan["lds"] == RAY_QUEUE * plan["waves_per_pixel"] + lds
    want, ws = sc.render(flux, sd, 128, DEPTH, SEED, flux.KERNEL_REFILL)[:2]
    assert gs == ws and np.abs(got - want).max() <= TOL_ORDER
