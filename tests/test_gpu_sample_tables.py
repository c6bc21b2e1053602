"""The glossy lobe's angle table (RenderParams::glossx): per held sample and per distinct glossy exponent of the scene, the
(cos theta, sin theta) that fast_bounce otherwise computes at every glossy bounce.  The fill applies the loop's own operations, so a
context with the table and one built under FLUX_SAMPLE_TABLES=0 (read at context creation) must render the SAME BITS with the same
path statistics -- in the split kernel with its hit queue (256 spp: a one-wave block takes the queue under FLUX_SPLIT_HITQ_CAP /
FLUX_SPLIT_HITQ_TAKE_AT; 16384 spp on a few pixels: the plan's own), the refill kernel (64 spp) and the static kernel (16 spp), for
one, three and five exponents (five: past the cap, no table), exponent 0, and with and without a lens.  One case per kernel is also
held against the oracle at test_gpu_parity.py's bounds.  tests/sample_tables_selftest.cpp looks at the table itself."""
import copy

import numpy as np
import pytest

import selftest
import split_checks as sc
from conftest import max_abs_diff, small_scene
from split_checks import REC, SLOT, SPH, TOL_ORACLE
from switches import queue, switches  # noqa: F401 (the fixture)
from test_sample_table_slots import build_selftest

pytestmark = pytest.mark.gpu

TOL_TIGHT = 1e-9
DEPTH, SEED = 5, 3

# demo2's three exponents; one; five distinct ones (kGlossExpSlots = 4); exponent 0 beside another
# "plane": the floor glossy too, with an exponent of its own -- a record past the spheres (scan order) whose slot is not the first
EXPONENTS = {"one": [100.0], "three": [10000.0, 100.0, 10.0], "five": [10000.0, 100.0, 10.0, 3.0, 30.5], "zero": [0.0, 100.0],
             "plane": [100.0]}
PLANE_EXPONENT = 25.0
HAS_TABLE = {"one": True, "three": True, "five": False, "zero": True, "plane": True}
KERNEL_OF_ROOT = {16: "PLAN_SPLIT", 8: "PLAN_REFILL", 4: "PLAN_STATIC"}


def _scene(flux, demo2, name, lens):
    """demo2's camera, environment and plane around a handful of its spheres, every second one glossy with the case's exponents in turn, the others Matte."""
    sd = copy.deepcopy(small_scene(demo2, 32, 24))
    env = next(s for s in sd.shapes if isinstance(s, flux.SphereData) and s.invert)
    planes = [s for s in sd.shapes if isinstance(s, flux.PlaneData)]
    spheres = [s for s in sd.shapes if isinstance(s, flux.SphereData) and not s.invert][:10]
    exps = EXPONENTS[name]
    for k, s in enumerate(spheres):
        if k % 2 == 0:
            s.material = flux.GlossyReflectiveData(0.8, (0.9, 0.85, 0.8), exps[(k // 2) % len(exps)])
        else:
            s.material = flux.MatteData((0.7, 0.6, 0.5), (0, 0, 0), 0.8)
    if name == "plane":
        for p in planes:
            p.material = flux.GlossyReflectiveData(0.6, (0.8, 0.8, 0.9), PLANE_EXPONENT)
    sd.shapes = [env] + spheres + planes
    sd.camera_data.lens_radius = lens
    return sd


@pytest.mark.parametrize("lens", [0.0, 0.3])
@pytest.mark.parametrize("root", [16, 8, 4])
@pytest.mark.parametrize("name", ["one", "three", "five", "zero", "plane"])
def test_frames_do_not_depend_on_the_table(flux, demo2, switches, name, root, lens):
    sd = _scene(flux, demo2, name, lens)
    q = queue((80, 16) if root == 16 else None)  # a one-wave block's LDS holds 88 slots for this scene: the plan takes the hit queue from H = 24 down
    switches(**q)
    got, gs, gplan, gbytes = sc.render(flux, sd, root, DEPTH, SEED)[:4]
    switches(FLUX_SAMPLE_TABLES=0, **q)
    want, ws, wplan, wbytes = sc.render(flux, sd, root, DEPTH, SEED)[:4]
    switches(**q)
    assert gplan["kernel"] == wplan["kernel"] == getattr(flux._lib, KERNEL_OF_ROOT[root])
    if root == 16:
        # the hit queue (68 B a slot), both times -- not the ray queue (5120 B a wave)
        queues = gplan["lds"] - (len(sd.shapes) * REC + sum(isinstance(s, flux.SphereData) for s in sd.shapes) * SPH)
        assert gplan["lds"] == wplan["lds"] and gplan["waves_per_pixel"] == 1 and queues == 80 * SLOT
    assert gs["glossy_bounces"] > 0 and gs == ws
    assert np.array_equal(got, want)
    # the context reports the table by the memory it holds: one entry of 16 B per held sample and exponent, or nothing
    slots = 2 if name == "plane" else {1: 1, 2: 2, 3: 3, 5: 0}[len(EXPONENTS[name])]
    assert (slots > 0) == HAS_TABLE[name]
    table = 32 * root * root * 16 * slots + ((len(sd.shapes) + 1) * 4 if slots else 0)
    assert gbytes - wbytes == table


def test_headline_plan_reads_the_table(flux, demo2, switches):
    """16384 spp, the plan's own hit queue (four waves a pixel, 110 slots of 68 B a wave for demo2's records), demo2 itself."""
    sd = small_scene(demo2, 8, 6)
    got, gs, gplan, gbytes = sc.render(flux, sd, 128, DEPTH, SEED)[:4]
    switches(FLUX_SAMPLE_TABLES=0)
    want, ws, wplan, wbytes = sc.render(flux, sd, 128, DEPTH, SEED)[:4]
    assert gplan["kernel"] == wplan["kernel"] == flux._lib.PLAN_SPLIT and gplan["waves_per_pixel"] == 4
    n_sph = sum(isinstance(s, flux.SphereData) for s in sd.shapes)
    assert gplan["lds"] == wplan["lds"] == 110 * SLOT * 4 + len(sd.shapes) * REC + n_sph * SPH
    assert gs["glossy_bounces"] > 0 and gs == ws
    assert np.array_equal(got, want)
    assert gbytes - wbytes == 8 * 16384 * 48 + (len(sd.shapes) + 1) * 4


_oracle = {}   # the oracle's frame and statistics per sample root and scene


@pytest.mark.parametrize("root", [16, 8, 4])
def test_against_the_oracle(flux, oracle_mod, demo2, switches, root):
    sd = _scene(flux, demo2, "three", 0.3)
    want, ost = sc.references(_oracle, (root, "three"), flux, oracle_mod, sd, root, DEPTH, SEED, kernels=())
    switches(**queue((80, 16) if root == 16 else None))  # the hit queue, as above
    got, gs, plan = sc.render(flux, sd, root, DEPTH, SEED)[:3]
    assert plan["kernel"] == getattr(flux._lib, KERNEL_OF_ROOT[root])
    assert {k: gs[k] for k in ost} == ost
    assert max_abs_diff(got, want) < TOL_ORACLE
    assert np.percentile(np.abs(got - want), 99.9) < TOL_TIGHT


def test_glossy_plane_against_the_oracle(flux, oracle_mod, demo2, switches):
    """The glossy floor: most primary hits read the table through a record behind the spheres'."""
    sd = _scene(flux, demo2, "plane", 0.3)
    want, ost = sc.references(_oracle, (8, "plane"), flux, oracle_mod, sd, 8, DEPTH, SEED, kernels=())
    got, gs = sc.render(flux, sd, 8, DEPTH, SEED)[:2]
    assert {k: gs[k] for k in ost} == ost
    assert max_abs_diff(got, want) < TOL_ORACLE
    assert np.percentile(np.abs(got - want), 99.9) < TOL_TIGHT


def test_table_entries_and_set_share(tmp_path):
    exe = build_selftest(tmp_path)
    out = selftest.run(exe, "gpu", timeout=60)
    for name in ("table values", "set rows", "set share", "one exponent", "past the cap", "switch"):
        assert f"ok {name}" in out
    assert "all ok" in out
