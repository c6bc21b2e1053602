"""The split kernel's instantiations swept over generated scenes (tests/split_sweep.py: nine classes of six scenes, each built to be in
its class; tests/test_split_sweep.py shows on the CPU that they are worth rendering).  One test a scene; both of its jobs -- root
128 at depth 5 (four waves a pixel, the benchmark's job) and one of split_sweep.JOBS -- run in FAST with the plan's own settings:

  flags     launch_plan(flags=True) says PLAN_SPLIT, the job's waves a pixel and the very instantiation split_sweep.expected_flags restates
            from the planner's rules (word 7 of flux_ctx_launch_plan: TYP, MAX32, the axis, hit queue, table, cut, copy).
  oracle    the seven classes the CPU oracle knows, at the job's FULL sample count: every path statistic of the oracle equal, the
            finiteness pattern equal, finite pixels within 1e-4 (the project's FAST-to-reference bound, tests/test_gpu_plane_axis.py).
  kernels   split, refill and static on the same job: statistics equal, |split - static| and |split - refill| <= 1e-12 (the same
            samples in another summation order); the instantiation without statistics gives the same frame bits as the one with.
  disks, boxes and glass: the static kernel at 64 spp against tests/path_spec.py (test_gpu_ext_fuzz.check_run), then the chain above
            from the static kernel at the full count, as test_gpu_ext_fuzz.test_two_and_four_waves_a_pixel.
  switches  the first two scenes of a class, the root-128 job, each switch set before the context is created and held to what its
            own test file asserts on demo2: FLUX_SPLIT_HITQ_CAP=0 and FLUX_SPLIT_HITQ_TAKE_AT=32 within 1e-12 of the static and
            refill kernels (test_gpu_split_hit_queue.py); FLUX_SPLIT_DEPTH_CUT=0 within 1e-12 of the frame with the cut
            (test_gpu_depth_cut.py); FLUX_THROUGHPUT_TABLE=0, FLUX_PLANE_AXIS=0, FLUX_SPLIT_UNIFORM_A=0 and FLUX_SAMPLE_TABLES=0 the
            same bits (test_gpu_throughput_table.py, test_gpu_plane_axis.py, test_gpu_uniform_phase_a.py, test_gpu_sample_tables.py);
            equal statistics and the flags the switch leaves, every time.
  shares    the third scene of a class (5 x 3: three ranks hold 2, 2 and 1 sets, one row each) through a loopback MultiRenderer
            in both shard modes: the frame of render_frame, bit for bit.  (The library refuses set shares below 64 spp only.)

No scene is skipped, reseeded or excluded here, and no (scene, job) needed the allowance for FAST arithmetic differing from the
oracle: all 108 runs agree with it, or with the path reference, in every statistic.

Measured on an MI355X machine: the 54 tests take 7.3 s together; 0.77 and 0.70 s the two slowest (glass-5, disks_and_boxes-5:
8 x 6 pixels and the Python path reference at 64 spp), 0.26 s the slowest of the others (typ_axis-0, with its seven switches), 0.03
to 0.19 s the rest.  Worst figures: |split - oracle| 5.1e-13, |split - static| 6.8e-15, |split - refill| 1.0e-15.

Three arithmetic-only mutants of the library against this file: the throughput table's products of lists of three entries or more
times 1 + 1e-6 -- 31 tests fail (all thirty scenes of typ_axis, typ_no_axis, no_env_shortcut, beyond_the_guard and five_exponents,
whose headline job reads the table, and disks_and_boxes-2); the Reflective weight of a taken hit times 1 + 1e-6 -- 31 fail, in
every class but glass, which has no hit queue (the scenes with a mirror in a hit-queue job); the z branch of plane_axis_num_den times
1 + 2^-40 -- none fails, here or in test_gpu_plane_axis.py.  A path's value is a product of per-record weights and an emitter's colour: a frame is piecewise constant in the geometry, and no frame can see a change
of t smaller than the gap to the next decision.  tests/test_plane_axis.py compiles the same header for the host and fails on that
mutant at its first -z ray.
"""
import numpy as np
import pytest

import split_checks as sc
import split_sweep as sw
from split_checks import TOL_ORACLE, TOL_ORDER
from switches import switches  # noqa: F401 (the fixture)
from test_gpu_ext_fuzz import check_run

pytestmark = pytest.mark.gpu

# switch -> (value, how the frame is held: "order" = within 1e-12 of the static and refill kernels, "cut" = within 1e-12 of the
# plan's own frame, "bits" = that frame's bits)
SWITCHES = {"FLUX_SPLIT_HITQ_CAP": ("0", "order"), "FLUX_SPLIT_HITQ_TAKE_AT": ("32", "order"), "FLUX_THROUGHPUT_TABLE": ("0", "bits"),
            "FLUX_SPLIT_DEPTH_CUT": ("0", "cut"), "FLUX_PLANE_AXIS": ("0", "bits"), "FLUX_SPLIT_UNIFORM_A": ("0", "bits"),
            "FLUX_SAMPLE_TABLES": ("0", "bits")}


def _check_plan(flux, plan, sd, root, depth, tag, env=None):
    want = sw.expected_flags(flux, sd, root, depth, env)
    print(f"{tag}: plan {sw.describe(flux, plan['flags'])}, K {plan['waves_per_pixel']}, lds {plan['lds']}")
    assert plan["kernel"] == flux._lib.PLAN_SPLIT and plan["waves_per_pixel"] == sw.waves_per_pixel(root), (tag, plan)
    assert plan["math"] == flux.MATH_FAST and plan["route"] == flux._lib.ROUTE_NONE, (tag, plan)
    assert plan["flags"] == want, f"{tag}: the plan says {sw.describe(flux, plan['flags'])}, expected {sw.describe(flux, want)}"
    cap = sw.plan_hitq(flux, sd, root, depth, env)[0]
    assert plan["lds"] == (cap * sc.SLOT if cap else sc.RAY_QUEUE) * plan["waves_per_pixel"] + sc.scene_lds(flux, sd), (tag, plan)


@pytest.mark.parametrize("index", range(sw.SCENES_PER_CLASS))
@pytest.mark.parametrize("cls", sw.CLASSES)
def test_split_kernel_on_a_generated_scene(flux, switches, cls, index):
    sd, seed = sw.scene(cls, index)
    draw = sw.DRAWS.get(cls, {}).get(index, 0)
    headline = {}
    for root, depth in sw.jobs_of(index):
        tag = f"{cls} {index} root {root} depth {depth}"
        if cls not in sw.ORACLE_CLASSES:   # the link to the path reference: the static kernel at 64 spp
            with flux.Renderer(sd, flux.JobConfiguration(8, depth, 50), seed=seed) as r:
                r.set_kernel(flux.KERNEL_STATIC)
                check_run(flux, r, sw.path_run(cls, index, draw, depth), f"{tag}: static kernel at 64 spp", True, {})
        with flux.Renderer(sd, flux.JobConfiguration(root, depth, 50), seed=seed) as r:
            static, ss = sc.with_stats(flux, r, flux.KERNEL_STATIC)
            refill, rs = sc.with_stats(flux, r, flux.KERNEL_REFILL)
            plain, got, gs, plan = sc.split_run(flux, r)
        _check_plan(flux, plan, sd, root, depth, tag)
        err_static, err_refill = sc.distance(got, static), sc.distance(got, refill)
        print(f"{tag}: |split - static| {err_static:.3e}  |split - refill| {err_refill:.3e}  segments {gs['segments']}  "
              f"depth_exhausted {gs['depth_exhausted']}")
        if cls in sw.ORACLE_CLASSES:
            want, ost, _ = sw.oracle_run(cls, index, draw, root, depth)
            differing = {k: (gs[k], ss[k], rs[k], ost[k]) for k in ost if not gs[k] == ss[k] == rs[k] == ost[k]}
            assert not differing, f"{tag}: statistics (split, static, refill, oracle) {differing}"
            err_oracle = sc.distance(got, want)
            print(f"{tag}: |split - oracle| {err_oracle:.3e}")
            assert err_oracle < TOL_ORACLE, tag
        assert gs == ss == rs, (tag, gs, ss, rs)
        assert err_static <= TOL_ORDER and err_refill <= TOL_ORDER, tag
        assert sc.same_bits(plain, got), f"{tag}: the instantiation without statistics renders other bits"
        if (root, depth) == sw.HEADLINE_JOB:
            headline = dict(static=static, refill=refill, got=got, plain=plain, stats=gs)

    root, depth = sw.HEADLINE_JOB
    cfg = flux.JobConfiguration(root, depth, 50)
    if index < 2:
        for name, (value, how) in SWITCHES.items():
            tag = f"{cls} {index} {name}={value}"
            switches(**{name: value})   # before the context: its tables are made at creation
            try:
                with flux.Renderer(sd, cfg, seed=seed) as r:
                    plain, img, st, plan = sc.split_run(flux, r)
            finally:
                switches()
            _check_plan(flux, plan, sd, root, depth, tag, {name: value})
            assert st == headline["stats"], (tag, st, headline["stats"])
            assert sc.same_bits(plain, img), tag
            if how == "bits":
                assert sc.same_bits(img, headline["got"]) and sc.same_bits(plain, headline["plain"]), f"{tag}: the switch changes bits"
            elif how == "cut":
                err = sc.distance(img, headline["got"])
                print(f"{tag}: |uncut - cut| {err:.3e}")
                assert err <= TOL_ORDER, tag
            else:
                err = max(sc.distance(img, headline["static"]), sc.distance(img, headline["refill"]))
                print(f"{tag}: |split - static or refill| {err:.3e}")
                assert err <= TOL_ORDER, tag
    if index == 2:
        for mode in (flux._lib.SHARD_SETS, flux._lib.SHARD_ROWS):
            with flux.MultiRenderer(sd, cfg, seed=seed, devices=[0] * 3, shard=mode | flux._lib.SHARD_LOOPBACK) as m:
                frame = m.render_frame()
            assert sc.same_bits(np.ascontiguousarray(frame), headline["plain"]), f"{cls} {index}: three ranks, shard mode {mode}"
