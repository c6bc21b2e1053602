"""The split kernel's take of a parked hit reads the path's throughput from the scene's product table (flux_plan.h tput_index;
DESIGN.md section 3) where the context holds one, and multiplies it up from the bounce list where it does not; the hit queue's slot
keeps its doubles on even dwords.  Neither changes an operation on a value that reaches the image, so the split kernel is held to what
tests/test_gpu_hitq_classes.py holds it to -- the path statistics equal the oracle's (the static kernel's for a scene the oracle does
not know) and the image within 1e-12 of the static kernel's (the summation order) -- and the frame with the table is the frame
without it (FLUX_THROUGHPUT_TABLE=0), bit for bit.

8 x 6 pixels, at 16384 spp (four waves a pixel) and at sample root 91 (8281 spp: two waves a pixel, a smaller pool).  Scenes:
  demo2        13 records, 4 bits an entry: the table, at depth limits 5, 2 and 3 (lists of up to four, one and two entries)
  records16    demo2 and three small Matte spheres: 16 records, every 4-bit entry value in use
  records17    a fourth one: 17 records, 5 bits, 48 MiB at depth 5 -- no table, the loop
  box_room     5 bits: the loop at depth 5, the table at depth 3
Every case once more with FLUX_SPLIT_HITQ_TAKE_AT=32: thinner batches, which mix depths differently.
"""
import copy
import os

import numpy as np
import pytest

import split_checks as sc
from switches import switches as env_switches  # noqa: F401 (the fixture)
from conftest import SCENES, small_scene
from split_checks import SLOT, TOL_ORDER

pytestmark = pytest.mark.gpu

W, H, SEED = 8, 6, 1
# scene, depth limit -> whether the context holds a table
CASES = [("demo2", 5, True), ("demo2", 2, True), ("demo2", 3, True), ("records16", 5, True), ("records17", 5, False),
         ("box_room", 5, False), ("box_room", 3, True)]
NOT_IN_THE_ORACLE = ("box_room",)
ROOTS = {128: 4, 91: 2}  # sample root -> waves per pixel


@pytest.fixture(scope="module")
def scenes(flux, demo2):
    out = {"demo2": small_scene(demo2, W, H), "box_room": small_scene(flux.load_scene(os.path.join(SCENES, "box_room.yml")), W, H)}
    for extra in (3, 4):
        sd = copy.deepcopy(out["demo2"])
        for k in range(extra):  # in front of the row of spheres, each with a weight of its own
            m = flux.MatteData((0.2 + 0.2 * k, 0.9 - 0.15 * k, 0.35 + 0.1 * k), (1.0, 1.0, 1.0), 0.6 + 0.1 * k)
            sd.shapes.append(flux.SphereData((-3.0 + 2.0 * k, 0.5, -3.5), 0.5, m, False))
        out[f"records{13 + extra}"] = sd
    assert len(out["demo2"].shapes) == 13 and len(out["records16"].shapes) == 16 and len(out["records17"].shapes) == 17
    return out


@pytest.fixture
def env(env_switches):
    return lambda take_at=None, tables=True: env_switches(FLUX_SPLIT_HITQ_TAKE_AT=take_at, FLUX_THROUGHPUT_TABLE=None if tables else 0)


_refs = {}   # per scene, sample root and depth limit: the oracle's statistics and the static kernel's run


@pytest.mark.parametrize("take_at", [None, 32])
@pytest.mark.parametrize("n", sorted(ROOTS))
@pytest.mark.parametrize("name,depth,has_table", CASES)
def test_split_with_and_without_the_table(flux, oracle_mod, scenes, env, name, depth, has_table, n, take_at):
    sd = scenes[name]
    _, ost, (want, ws, *_) = sc.references(_refs, (name, n, depth), flux, oracle_mod, sd, n, depth, SEED, kernels=("STATIC",),
                                           oracle_sd=None if name in NOT_IN_THE_ORACLE else sc.SAME)
    env(take_at, tables=True)
    got, gs, plan, bytes_on = sc.render(flux, sd, n, depth, SEED, flux.KERNEL_SPLIT)[:4]
    env(take_at, tables=False)
    loop, ls, plan_off, bytes_off = sc.render(flux, sd, n, depth, SEED, flux.KERNEL_SPLIT)[:4]
    env()
    # the hit queue (C slots of 68 B a wave beside the scene's records), and the same plan with and without the table
    assert plan == plan_off and plan["kernel"] == flux._lib.PLAN_SPLIT and plan["waves_per_pixel"] == ROOTS[n]
    records = sum(6 if isinstance(s, flux.BoxData) else 1 for s in sd.shapes)  # a box: one record per face
    queues = (plan["lds"] - sc.scene_lds(flux, sd)) // plan["waves_per_pixel"]
    assert queues % SLOT == 0 and queues >= (64 + (take_at or 32)) * SLOT
    bits = (records - 1).bit_length()
    assert bits == (5 if name in ("records17", "box_room") else 4)
    # the table is an allocation of its own: its bytes are in the context's
    assert bytes_on - bytes_off == ((2 << bits * (depth - 1)) * 24 if has_table else 0)
    assert np.array_equal(got, loop) and gs == ls
    assert gs == ws
    if ost is not None:
        assert {k: ws[k] for k in ost} == ost and {k: gs[k] for k in ost} == ost
    assert gs["matte_bounces"] > 0
    assert np.abs(got - want).max() <= TOL_ORDER


def test_every_record_is_in_some_list(flux, scenes):
    """records16 uses every value a 4-bit list entry can take: each of its three added spheres is hit, and bounced off, in the
    frame (their Matte bounces are the ones demo2 does not have)."""
    a = sc.render(flux, scenes["demo2"], 128, 5, SEED, flux.KERNEL_SPLIT).stats
    b = sc.render(flux, scenes["records16"], 128, 5, SEED, flux.KERNEL_SPLIT).stats
    assert b["matte_bounces"] > a["matte_bounces"]
