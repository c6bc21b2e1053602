"""The BENCHMARKED configuration, exactly: scenes/demo2.yml, 800x600, sample_root 128 (16384 spp) -- the only sample
count at which a pixel's samples are split over FOUR waves (K = 4: slice bounds, the part[][] exchange through LDS, the
wave-order sum), and 9216 spp (sample_root 96), the smallest count with K = 2.

Camera::render (fluxcore/src/trace.rs:71-87) visits every sample of a pixel exactly once and multiplies the sum by
1/N.  Below 8192 spp a wave owns a whole pixel; from there on that is a property of the slicing code, and only an exact
comparison sees a slice bug that drops or doubles a few samples (one sample of 16384 moves a pixel by 6e-5 relative: inside
any Monte-Carlo comparison with demo.png, far outside 1e-9).  So, at these counts:

  (a) rows of the frame from the default kernel against the ORACLE (1e-4 per channel, the north-star tolerance; 1e-9 at
      the 99.9th percentile: what FP64 on both sides delivers);
  (b) the three kernels against each other -- split (K = 4) == refill (K = 4) == static (K = 1) to 1e-12, path statistics
      identical, in both arithmetics;
  (c) the call bench.py TIMES -- flux_render_sets_device(0, 1, 800) through SetSharder -- bit-equal to render_frame(),
      and the eight G = 8 shares (100 sets each: twelve full XCD groups plus the `set_count % 8 = 4` remainder deal of
      map_wave), rendered one after the other and reassembled, bit-equal to the same frame.

K is asked of the library's own launch planner (flux_ctx_launch_plan), not re-derived here, so this file fails if the
threshold moves again and the counts no longer reach K > 1 (as tests/test_triangles.py's did in round 2).
"""
import numpy as np
import pytest

from conftest import max_abs_diff
from extension_checks import set_sharded_frame

pytestmark = pytest.mark.gpu

TOL_IMAGE = 1e-4   # north_star tolerance (per channel)
TOL_TIGHT = 1e-9   # FP64 on both sides, same estimator
TOL_ORDER = 1e-12  # kernels differ only in the fixed order a pixel's samples are summed in

ROW_BLOCKS = [(0, 1), (299, 301), (599, 599)]  # top edge, the image centre (spheres, floor), bottom edge
ROWS = [r for a, b in ROW_BLOCKS for r in range(a, b + 1)]


def _render_blocks(r, blocks):
    return np.concatenate([r.render_rows(a, b) for a, b in blocks])


@pytest.fixture(scope="module")
def headline(flux, demo2):
    """ONE context of the headline configuration (2.9 GB of tables) for the whole module."""
    r = flux.Renderer(demo2, flux.JobConfiguration(128, 5, 50), seed=1)
    yield r
    r.close()


def test_plan_of_the_benchmarked_launch(flux, headline):
    """What bench.py's timed call launches: the split kernel, one block of 4 waves per pixel, grouped by sample set."""
    r = headline
    r.set_math(flux.MATH_FAST)
    r.set_kernel(flux.KERNEL_DEFAULT)
    rows, sets = r.launch_plan(), r.launch_plan(num_sets=800)
    for plan in (rows, sets):
        assert plan["kernel"] == flux._lib.PLAN_SPLIT and plan["waves_per_pixel"] == 4 and plan["block"] == 256
        assert plan["blocks"] == 800 * 600
    share = r.launch_plan(num_sets=100)   # one rank of eight
    assert share["kernel"] == flux._lib.PLAN_SPLIT and share["waves_per_pixel"] == 4
    assert share["blocks"] == 8 * (12 * 600 + (4 * 600 + 7) // 8)   # 12 sets per XCD slot + an eighth of the last 4 sets' rows
    r.set_kernel(flux.KERNEL_STATIC)
    assert r.launch_plan()["waves_per_pixel"] == 1 and r.launch_plan()["kernel"] == flux._lib.PLAN_STATIC
    r.set_kernel(flux.KERNEL_REFILL)
    assert r.launch_plan()["waves_per_pixel"] == 4 and r.launch_plan()["kernel"] == flux._lib.PLAN_REFILL
    r.set_kernel(flux.KERNEL_DEFAULT)
    r.set_math(flux.MATH_STRICT)   # STRICT has no split kernel
    assert r.launch_plan()["kernel"] == flux._lib.PLAN_REFILL and r.launch_plan()["waves_per_pixel"] == 4
    r.set_math(flux.MATH_FAST)


def test_headline_rows_against_the_oracle(flux, oracle_mod, demo2, headline):
    """(a) at 16384 spp: six rows of the real frame, default kernel (split, K = 4), FAST and STRICT, against the oracle."""
    o = oracle_mod.Oracle(demo2, flux.JobConfiguration(128, 5, 50), seed=1)
    o.stats(reset=True)
    want = o.render_row_list(ROWS, threads=len(ROWS))
    want_stats = o.stats()
    o.close()
    r = headline
    r.set_kernel(flux.KERNEL_DEFAULT)
    for math in (flux.MATH_FAST, flux.MATH_STRICT):
        r.set_math(math)
        assert r.launch_plan(num_rows=2)["waves_per_pixel"] == 4
        r.enable_stats(True)
        r.stats(reset=True)
        got = _render_blocks(r, ROW_BLOCKS)
        st = r.stats(reset=True)
        r.enable_stats(False)
        assert got.shape == want.shape == (len(ROWS), 800, 3)
        d = np.abs(got - want)
        assert d.max() < TOL_IMAGE, (math, d.max())
        assert np.percentile(d, 99.9) < TOL_TIGHT, (math, np.percentile(d, 99.9))
        # every sample exactly once (trace.rs:71-87), every decision the oracle's
        assert st["samples"] == len(ROWS) * 800 * 16384
        assert {k: st[k] for k in want_stats} == want_stats, math
    r.set_math(flux.MATH_FAST)


def test_two_waves_per_pixel_rows_against_the_oracle(flux, oracle_mod, demo2):
    """(a) at 9216 spp (sample_root 96: K = 2), two rows."""
    cfg = flux.JobConfiguration(96, 5, 50)
    o = oracle_mod.Oracle(demo2, cfg, seed=1)
    o.stats(reset=True)
    want = o.render_row_list([300, 599], threads=2)
    want_stats = o.stats()
    o.close()
    with flux.Renderer(demo2, cfg, seed=1) as r:
        plan = r.launch_plan(num_rows=1)
        assert plan["kernel"] == flux._lib.PLAN_SPLIT and plan["waves_per_pixel"] == 2
        r.enable_stats(True)
        r.stats(reset=True)
        got = _render_blocks(r, [(300, 300), (599, 599)])
        st = r.stats()
        d = np.abs(got - want)
        assert d.max() < TOL_IMAGE and np.percentile(d, 99.9) < TOL_TIGHT, (d.max(), np.percentile(d, 99.9))
        assert {k: st[k] for k in want_stats} == want_stats
        r.enable_stats(False)
        r.set_kernel(flux.KERNEL_STATIC)   # K = 1 at the same count
        assert max_abs_diff(got, _render_blocks(r, [(300, 300), (599, 599)])) < TOL_ORDER


def test_kernels_agree_at_four_waves_per_pixel(flux, headline):
    """(b) split (K = 4) == refill (K = 4) == static (K = 1) on the six rows at 16384 spp: images to 1e-12 (the fixed
    summation orders differ), statistics identical -- in FAST; refill == static in STRICT; FAST == STRICT to 1e-9."""
    r = headline
    out, stats = {}, {}
    combos = [(flux.MATH_FAST, flux.KERNEL_SPLIT, flux._lib.PLAN_SPLIT, 4), (flux.MATH_FAST, flux.KERNEL_REFILL, flux._lib.PLAN_REFILL, 4),
              (flux.MATH_FAST, flux.KERNEL_STATIC, flux._lib.PLAN_STATIC, 1), (flux.MATH_STRICT, flux.KERNEL_REFILL, flux._lib.PLAN_REFILL, 4),
              (flux.MATH_STRICT, flux.KERNEL_STATIC, flux._lib.PLAN_STATIC, 1)]
    r.enable_stats(True)
    for math, variant, kernel, K in combos:
        r.set_math(math)
        r.set_kernel(variant)
        plan = r.launch_plan(num_rows=3)
        assert plan["kernel"] == kernel and plan["waves_per_pixel"] == K, plan
        r.stats(reset=True)
        out[(math, variant)] = _render_blocks(r, ROW_BLOCKS)
        stats[(math, variant)] = r.stats(reset=True)
    r.enable_stats(False)
    r.set_math(flux.MATH_FAST)
    r.set_kernel(flux.KERNEL_DEFAULT)
    ref = out[(flux.MATH_STRICT, flux.KERNEL_STATIC)]
    assert stats[(flux.MATH_STRICT, flux.KERNEL_STATIC)]["samples"] == len(ROWS) * 800 * 16384
    for key, img in out.items():
        assert stats[key] == stats[(flux.MATH_STRICT, flux.KERNEL_STATIC)], key
        assert np.isfinite(img).all()
        tol = TOL_ORDER if key[0] == flux.MATH_STRICT else TOL_TIGHT
        assert max_abs_diff(img, ref) < tol, (key, max_abs_diff(img, ref))
    fast_static = out[(flux.MATH_FAST, flux.KERNEL_STATIC)]
    for variant in (flux.KERNEL_SPLIT, flux.KERNEL_REFILL):
        assert max_abs_diff(out[(flux.MATH_FAST, variant)], fast_static) < TOL_ORDER, variant
    # product build (no statistics: another instantiation of the kernel templates): the same pixels, bit for bit
    assert np.array_equal(_render_blocks(r, ROW_BLOCKS), out[(flux.MATH_FAST, flux.KERNEL_SPLIT)])


@pytest.mark.parametrize("n", [32, 128])
def test_the_call_bench_times_equals_render_frame(flux, demo2, headline, n):
    """(c) 800x600 at 1024 and 16384 spp: SetSharder over flux_render_sets_device -- world 1 is bench.py's timed call,
    world 8 the eight shares of a SCALE run (100 sets each) -- against the row-based frame, bit for bit."""
    import torch
    r = headline if n == 128 else flux.Renderer(demo2, flux.JobConfiguration(n, 5, 50), seed=1)
    try:
        r.set_math(flux.MATH_FAST)
        r.set_kernel(flux.KERNEL_DEFAULT)
        full = torch.from_numpy(r.render_frame())
        assert torch.isfinite(full).all()
        assert torch.equal(set_sharded_frame(flux, r, 1, check_plan=True), full)
        assert torch.equal(set_sharded_frame(flux, r, 8, check_plan=True), full)
        # ... and the row tiles of `bench.py --shard rows` (FrameSharder: rows g, g + 8, ...)
        from flux_amd.dist import FrameSharder, hip_render_fn
        dev = torch.device("cuda", 0)
        shards = []
        for rank in range(8):
            sh = FrameSharder(r.height, r.width, rank, 8, dev)
            sh.render(hip_render_fn(r))
            torch.cuda.synchronize()
            shards.append(sh)
        s0 = shards[0]
        s0.gathered.copy_(torch.stack([s.local for s in shards]))
        assert torch.equal(s0.assemble().cpu(), full)
    finally:
        if r is not headline:
            r.close()
