"""The split kernel traces a pixel's samples in the order of the set's table (flux_amd/csrc/flux_sample_order.h, TABLE_ORDER): sorted by
the first-bounce direction of a stored-normal Matte hit, hemi[set][0][i], and dealt over the four quarters of the row.  Phase A reads the
primary ray's two tables from the set's copies in that order (DevSetRows::pix_o, disc_o), everything else by the sample index.

  table     (first in the file: before any render) sample roots 8, 9, 16, 17 and 128: every held set's row is a permutation of
            0 .. N-1; two contexts build the same table; a set-share context (rank 1 of 3) holds the rows of the full context's sets
            1, 4, 7, ...; each row equals the numpy restatement (tests/sample_order_ref.py) applied to table(TABLE_HEMI);
            FLUX_SAMPLE_ORDER=0 gives the identity.
  renders   three scenes -- a floor under an environment, as demo2; glossy spheres without a floor; no environment -- on the job list
            of tests/split_sweep.py plus roots 16 and 17 at depth 5, frames of 5 x 3, 4 x 3 and 7 x 3 pixels.  With the hit queue (the
            plan's own choice), with FLUX_SPLIT_HITQ_CAP=0 (the ray queue) and with FLUX_SPLIT_UNIFORM_A=0: all eight path statistics
            equal the CPU oracle's at the full sample count, the finiteness pattern equals the oracle's, finite pixels within 1e-4;
            against the same context under FLUX_SAMPLE_ORDER=0, and against the refill and static kernels: statistics equal, frames
            within 1e-12 (the same samples in another summation order); the instantiation without statistics gives the bits of the
            one with.
  waves     the jobs run 1, 2 and 4 waves a pixel (launch_plan).
  shares    three loopback ranks in both shard modes: the bits of render_frame.
"""
import copy
import functools

import numpy as np
import pytest

import sample_order_ref as ref
import split_checks as sc
import split_sweep as sw
from split_checks import TOL_ORACLE, TOL_ORDER
from switches import switches  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu

JOBS = sw.JOBS + ((16, 5), (17, 5))
SCENE_NAMES = ("floor", "glossy_no_floor", "no_environment")
FRAMES = {"floor": (5, 3), "glossy_no_floor": (4, 3), "no_environment": (7, 3)}
MODES = ({}, {"FLUX_SPLIT_HITQ_CAP": "0"}, {"FLUX_SPLIT_UNIFORM_A": "0"})


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(scene, seed): never written to"""
    import flux_amd as flux
    rng = np.random.default_rng(41000 + SCENE_NAMES.index(name))
    base = sw._base()
    if name == "floor":   # an environment, spheres of every material, a Matte floor with the normal +y
        sd = sw._analytic(flux, base, rng, FRAMES[name], 2, 6, "axis", 0)
    elif name == "glossy_no_floor":   # a cluster of glossy spheres that fills the view
        glossy = [flux.GlossyReflectiveData(float(rng.uniform(0.4, 1.0)), sw._color(rng, 0.3), e) for e in (1.0, 10.0, 100.0) * 3]
        sd = sw._analytic(flux, base, rng, FRAMES[name], 1, 9, None, 0, exponents=(1.0, 10.0, 100.0), materials=glossy, reach=1.8,
                          radii=(0.8, 1.6), lamp=False)
    else:   # no inverted sphere: a lamp, a floor, a coloured background
        light = flux.EmissiveData(sw._color(rng, 0.3), 2.0)
        sd = sw._analytic(flux, base, rng, FRAMES[name], 0, 7, "axis", 0, environment=False, materials=[light])
        sd.background = sw._f3(rng.uniform(0.1, 1.5, 3))
    return sd, int(rng.integers(1, 1 << 30))


_oracle = {}   # the oracle's frame and statistics per scene and job


# ---- (a) the table: before any render in this file ---------------------------------------------------------------------------------

@pytest.mark.parametrize("root", (8, 9, 16, 17, 128))
def test_table_is_the_restated_order_of_the_hemi_rows(flux, switches, root):
    sd = copy.deepcopy(_scene("no_environment")[0])   # 7 sets: rank 1 of 3 holds sets 1 and 4
    cfg = flux.JobConfiguration(root, 3, 50)
    N, T = root * root, flux._lib.TABLE_ORDER
    with flux.Renderer(sd, cfg, seed=11) as full, flux.Renderer(sd, cfg, seed=11) as again, \
            flux.Renderer(sd, cfg, seed=11, set_share=(1, 3)) as part:
        order, hemi = full.table(T), full.table(flux._lib.TABLE_HEMI)
        assert order.shape == (7, N) and hemi.shape == (7, 3, N, 3)
        assert np.array_equal(np.sort(order, axis=1), np.broadcast_to(np.arange(N, dtype=np.float64), (7, N))), "a row is no permutation"
        assert np.array_equal(again.table(T), order), "two contexts build different tables"
        assert np.array_equal(part.table(T), order[1::3]), "a set share holds other rows"
        for s in range(7):
            assert np.array_equal(order[s], ref.row_from_hemi(hemi[s, 0])), f"set {s}: not the restated order"
        if N % 256 == 0:   # every 64-aligned batch is one run of the sorted sequence: its keys ascend
            keys = ref.key(hemi[0, 0, :, 0], hemi[0, 0, :, 1])[order[0].astype(np.int64)].reshape(-1, 64)
            assert np.all(np.diff(keys.astype(np.int64), axis=1) >= 0)
        assert not np.array_equal(order[0], np.arange(N))
    switches(FLUX_SAMPLE_ORDER="0")
    with flux.Renderer(sd, cfg, seed=11) as off:
        assert np.array_equal(off.table(T), np.broadcast_to(np.arange(N, dtype=np.float64), (7, N)))


# ---- (b) renders -------------------------------------------------------------------------------------------------------------------

def test_jobs_run_one_two_and_four_waves_a_pixel(flux, switches):
    sd, seed = _scene("floor")
    seen = set()
    for root, depth in JOBS:
        with flux.Renderer(sd, flux.JobConfiguration(root, depth, 50), seed=seed) as r:
            r.set_kernel(flux.KERNEL_SPLIT)
            plan = r.launch_plan()
        assert plan["kernel"] == flux._lib.PLAN_SPLIT, (root, depth, plan)
        assert plan["waves_per_pixel"] == sw.waves_per_pixel(root), (root, depth, plan)
        seen.add(plan["waves_per_pixel"])
    assert seen == {1, 2, 4}


@pytest.mark.parametrize("job", JOBS, ids=lambda j: f"root{j[0]}-depth{j[1]}")
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_sorted_order_renders_the_same_samples(flux, oracle_mod, switches, name, job):
    root, depth = job
    sd, seed = _scene(name)
    cfg = flux.JobConfiguration(root, depth, 50)
    want, ost = sc.references(_oracle, (name, root, depth), flux, oracle_mod, sd, root, depth, seed, kernels=())
    for mode in MODES:
        tag = f"{name} root {root} depth {depth} {mode}"
        switches(**mode)
        try:
            with flux.Renderer(sd, cfg, seed=seed) as r:
                static, ss = sc.with_stats(flux, r, flux.KERNEL_STATIC)
                refill, rs = sc.with_stats(flux, r, flux.KERNEL_REFILL)
                plain, got, gs, plan = sc.split_run(flux, r)
            switches(FLUX_SAMPLE_ORDER="0", **mode)
            with flux.Renderer(sd, cfg, seed=seed) as r:
                plain0, got0, gs0, plan0 = sc.split_run(flux, r)
        finally:
            switches()
        assert plan["kernel"] == flux._lib.PLAN_SPLIT and plan["waves_per_pixel"] == sw.waves_per_pixel(root), (tag, plan)
        assert plan == plan0, f"{tag}: the switch changes the plan"   # (no bit of the flags word belongs to the order)
        hitq = bool(plan["flags"] & flux._lib.PLAN_FLAG_HITQ)
        if "FLUX_SPLIT_HITQ_CAP" in mode:
            assert not hitq, tag
        assert bool(plan["flags"] & flux._lib.PLAN_FLAG_UNIFORM_A) == ("FLUX_SPLIT_UNIFORM_A" not in mode), tag
        err = dict(oracle=sc.distance(got, want), index_order=sc.distance(got, got0), static=sc.distance(got, static), refill=sc.distance(got, refill))
        print(f"{tag}: hit queue {hitq}  " + "  ".join(f"|sorted - {k}| {v:.3e}" for k, v in err.items()) + f"  segments {gs['segments']}")
        differing = {k: (gs[k], gs0[k], ss[k], rs[k], ost[k]) for k in ost if not gs[k] == gs0[k] == ss[k] == rs[k] == ost[k]}
        assert len(ost) == 8 and not differing, f"{tag}: statistics (sorted, index order, static, refill, oracle) {differing}"
        assert gs == gs0 == ss == rs, (tag, gs, gs0, ss, rs)
        assert err["oracle"] < TOL_ORACLE, tag
        assert err["index_order"] <= TOL_ORDER and err["static"] <= TOL_ORDER and err["refill"] <= TOL_ORDER, tag
        assert sc.distance(got0, want) < TOL_ORACLE, tag
        assert sc.same_bits(plain, got), f"{tag}: the instantiation without statistics renders other bits"
        assert sc.same_bits(plain0, got0), f"{tag}: (index order) the instantiation without statistics renders other bits"


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_three_loopback_ranks_render_the_same_bits(flux, switches, name):
    sd, seed = _scene(name)
    cfg = flux.JobConfiguration(*sw.HEADLINE_JOB, 50)
    with flux.Renderer(sd, cfg, seed=seed) as r:
        r.set_kernel(flux.KERNEL_SPLIT)
        want = r.render_frame()
    for mode in (flux._lib.SHARD_SETS, flux._lib.SHARD_ROWS):
        with flux.MultiRenderer(sd, cfg, seed=seed, devices=[0] * 3, shard=mode | flux._lib.SHARD_LOOPBACK) as m:
            frame = m.render_frame()
        assert sc.same_bits(np.ascontiguousarray(frame), want), f"{name}: three ranks, shard mode {mode}"
