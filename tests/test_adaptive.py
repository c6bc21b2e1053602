"""Adaptive sampling without a GPU: the numpy specification (tests/adaptive_spec.py) and its properties, the
conditions the GPU suite's cases must meet, the quality table recomputed from tests/path_spec.py's samples, the argument checks of
the two entry points that need no context (they run before any device call), the Python names, flux_host's helpers and the
`flux --adaptive` flags.  The kernels: tests/test_gpu_adaptive.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adaptive_spec as asp
import denoise_moments_spec as dms
import denoise_spec
import moments_spec as ms
from conftest import ROOT, SCENES, small_scene
import selftest
from extension_checks import host_bins
from path_spec import aov_buffers, PathSpec

H, W, N = 6, 8, 4


# ---- the rule on synthetic samples ---------------------------------------------------------------------------------------------------

class Noise:
    """A sampler of its own: pass c of pixel (y, x) is `base` plus a fixed random draw scaled by sigma[y, x], and exactly black where
    sigma is 0 (so that such a pixel's sums carry no rounding at all); records what was asked."""

    def __init__(self, sigma, seed=1, base=0.5):
        self.sigma, self.seed, self.base, self.asked = np.asarray(sigma, dtype=np.float64), seed, base, []

    def __call__(self, ys, xs, cs):
        out = np.empty((len(ys), N, 3))
        for j, (y, x, c) in enumerate(zip(ys, xs, cs)):
            self.asked.append((int(y), int(x), int(c)))
            rng = np.random.default_rng([self.seed, int(y), int(x), int(c)])
            out[j] = self.base + self.sigma[y, x] * (rng.random((N, 1)) - 0.5) if self.sigma[y, x] > 0.0 else 0.0
        return out


def test_one_pass_is_the_sample_moments_bit_for_bit():
    noise = Noise(np.full((H, W), 0.4))
    res = asp.adaptive(noise, H, W, N, threshold=0.0, max_passes=1)
    rad = np.stack([noise([y] * W, list(range(W)), [0] * W) for y in range(H)])
    assert res.moments.tobytes() == ms.from_samples(rad).tobytes()
    assert np.all(res.passes == 1) and len(res.active) == 1 and res.hot == []


def test_a_threshold_nothing_exceeds_gives_min_passes_everywhere():
    for min_passes in (1, 3):
        res = asp.adaptive(Noise(np.full((H, W), 0.4)), H, W, N, threshold=1e6, min_passes=min_passes, max_passes=7)
        assert np.all(res.passes == min_passes) and len(res.active) == min_passes and len(res.hot) == 1 and not res.hot[0].any()


def test_threshold_zero_without_dilation_runs_exactly_the_pixels_whose_variance_never_vanishes():
    sigma = np.full((H, W), 0.3)
    sigma[1, 2] = sigma[4, 5] = sigma[0, 0] = 0.0   # all samples equal, in every pass: e² = 0 is not > 0
    res = asp.adaptive(Noise(sigma), H, W, N, threshold=0.0, max_passes=5, dilate=0)
    assert np.array_equal(res.passes == 5, sigma > 0.0) and np.all(res.passes[sigma == 0.0] == 1)
    assert np.all(res.moments[..., ms.S2][sigma == 0.0] == 0.0)


def test_a_zero_variance_pixel_beside_a_hot_one_is_active_through_dilation():
    sigma = np.zeros((H, W))
    sigma[2, 3] = 0.5
    for dilate in (0, 1, 2):
        res = asp.adaptive(Noise(sigma), H, W, N, threshold=0.0, max_passes=3, dilate=dilate)
        want = np.zeros((H, W), bool)
        want[max(2 - dilate, 0):2 + dilate + 1, max(3 - dilate, 0):3 + dilate + 1] = True
        assert np.array_equal(res.passes == 3, want) and np.all(res.passes[~want] == 1)
        assert np.array_equal(res.active[1], want) and int(res.hot[0].sum()) == 1
    # clipped at the call's edges, not wrapped
    sigma = np.zeros((H, W))
    sigma[0, W - 1] = 0.5
    res = asp.adaptive(Noise(sigma), H, W, N, threshold=0.0, max_passes=2, dilate=2)
    assert int((res.passes == 2).sum()) == 9 and np.all(res.passes[3:] == 1) and np.all(res.passes[:, :W - 3] == 1)
    assert np.array_equal(asp.dilated(res.hot[0], 2), res.active[1])


def test_a_nan_pixel_stops_after_min_passes_and_an_inf_stays_hot():
    class Poisoned(Noise):
        def __call__(self, ys, xs, cs):
            out = super().__call__(ys, xs, cs)
            for j, (y, x) in enumerate(zip(ys, xs)):
                if (y, x) == (1, 1):
                    out[j, 2, 0] = np.nan
                if (y, x) == (3, 4) and cs[j] == 0:
                    out[j, 1], out[j, 2] = 1e200, -1e200    # Σl = 0 and Σl² overflows: s² = inf over the floor, e² = inf
            return out
    res = asp.adaptive(Poisoned(np.zeros((H, W))), H, W, N, threshold=0.1, min_passes=2, max_passes=6, dilate=0)
    assert res.passes[1, 1] == 2 and np.isnan(res.moments[1, 1, ms.S2])
    assert res.passes[3, 4] == 6 and np.isposinf(res.moments[3, 4, ms.S2])
    assert int((res.passes == 2).sum()) == H * W - 1
    assert np.isfinite(res.decision_margin)  # the NaN and inf decisions are left out of the margin


def test_no_pixel_exceeds_max_passes_or_reads_a_set_twice():
    rng = np.random.default_rng(9)
    noise = Noise(rng.random((H, W)))
    S = W
    res = asp.adaptive(noise, H, W, N, threshold=0.01, max_passes=S, dilate=1)
    assert res.passes.max() == S and res.passes.min() >= 1
    per_pixel = {}
    for y, x, c in noise.asked:
        per_pixel.setdefault((y, x), []).append(c)
    set0 = rng.integers(0, S, (H, W))
    for (y, x), cs in per_pixel.items():
        assert cs == list(range(res.passes[y, x]))              # the pixel's OWN count, one pass each
        sets = [(set0[y, x] + c) % S for c in cs]
        assert len(set(sets)) == len(sets)                      # max_passes <= S: no set twice


def test_a_quiet_pixel_woken_by_a_neighbour_continues_with_its_own_count():
    """Row 0: D (x = 0) is hot throughout; B (x = 1) is flat in pass 0, so it takes pass 1 only through D, and noisy in pass 1, so
    it is hot from the second selection on; A (x = 2) is black, out of D's reach and within B's: quiet in round 1, woken in round 2,
    where it draws ITS pass 1 -- the round number would be 2."""
    asked = []

    def sampler(ys, xs, cs):
        out = np.zeros((len(ys), N, 3))
        for j, (y, x, c) in enumerate(zip(ys, xs, cs)):
            asked.append((int(y), int(x), int(c)))
            if (y, x) == (0, 0) or ((y, x) == (0, 1) and c >= 1):
                out[j, :, :] = np.array([0.0, 1.0, 0.0, 1.0])[:, None]
            elif (y, x) == (0, 1):
                out[j] = 0.5
        return out
    res = asp.adaptive(sampler, 1, W, N, threshold=0.1, max_passes=4, dilate=1)
    assert [a[0].tolist() for a in res.active] == [[True] * W, [True, True] + [False] * (W - 2), [True, True, True] + [False] * (W - 3),
                                                    [True, True, True] + [False] * (W - 3)]
    assert res.passes[0].tolist() == [4, 4, 3] + [1] * (W - 3)
    assert [c for y, x, c in asked if (y, x) == (0, 2)] == [0, 1, 2]


def test_finish_and_error2_keep_the_header_formulas():
    sums = np.array([[[2.0, 4.0, 1.0, 3.0, 2.5]]])
    c = np.array([[2]])
    mom = asp.finish(sums, c, N)
    n = 8.0
    assert np.array_equal(mom[0, 0, ms.MEAN], sums[0, 0, 0:3] * (1.0 / n))
    s2 = (2.5 - 9.0 / n) / (n - 1.0)
    assert mom[0, 0, ms.S2] == s2 and mom[0, 0, ms.VAR] == s2 / n
    assert asp.error2(sums[..., 3], sums[..., 4], c, N, 0.01)[0, 0] == (s2 / n) / ((3.0 / n) ** 2)
    assert asp.error2(np.array([0.0]), np.array([0.0]), np.array([1]), N, 0.01)[0] == 0.0
    dark = asp.error2(np.array([4e-3]), np.array([8e-6]), np.array([1]), N, 0.01)[0]   # m = 1e-3 < lum_floor: the floor divides
    assert dark == (((8e-6 - (4e-3 * 4e-3) / 4.0) / 3.0) / 4.0) / (0.01 * 0.01)


# ---- the GPU suite's cases ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(asp.CASES))
def test_gpu_case_conditions(flux, name):
    """What tests/test_gpu_adaptive.py relies on when it demands an EQUAL pass map: no hot decision within 1e-9 of the threshold
    (kernel and spec round e² differently by about 1e-15 (e² + 1/n), DESIGN.md section 5g's bound), no path decision at rounding
    level, and a run that exercises the rule: a pass map that is not constant, a pixel that stops early, one that reaches
    max_passes, one active only through dilation."""
    _, par, res = asp.case(flux, name)
    early, full, only_dilated, distinct = asp.counts(res, par)
    print(f"adaptive case {name}: tau {par['threshold']}, rounds {len(res.active)}, lists {[int(a.sum()) for a in res.active]}, mean passes "
          f"{res.passes.mean():.2f}; pixels that stop early {early}, at max_passes {full}, pixel-rounds active only through dilation "
          f"{only_dilated}, distinct counts {distinct}; decision margin {res.decision_margin:.2e}, path margin {res.path_margin:.2e}")
    assert res.decision_margin >= 1e-9
    assert res.path_margin >= ms.MIN_MARGIN
    assert distinct > 1 and early >= 1 and full >= 1 and only_dilated >= 1
    assert res.passes.max() <= par["max_passes"] and res.passes.min() >= par["min_passes"]
    assert np.isfinite(res.moments).all()


def test_gpu_special_cases(flux):
    """The two cases that cannot meet those conditions by what they are, with the property each is there for; and the lists that are
    no multiple of the pixels per wave."""
    _, par, single = asp.case(flux, "single-3x2")
    assert [int(a.sum()) for a in single.active][-1] == 1 and single.passes.shape == (2, 3)
    _, par1, round1 = asp.case(flux, "round1-2")
    assert len(round1.active) == 1 and len(round1.hot) == 1 and np.all(round1.passes == 1)
    for res in (single, round1):
        assert res.decision_margin >= 1e-9 and res.path_margin >= ms.MIN_MARGIN
    for name, ppw in (("open-2", 16), ("open-3", 7)):
        lists = [int(a.sum()) for a in asp.case(flux, name)[2].active]
        assert any(n % ppw for n in lists[1:]), (name, lists)
    wrap = asp.case(flux, "wrap-2")[2]
    assert wrap.passes.max() == 16 == ms.W  # every set of the 16 read once by some pixel: (set0 + c) % S wraps


def test_row_tiles_equal_the_frame_without_dilation(flux):
    tp = asp.traced(flux, "open", 2)
    par = dict(asp.DEFAULTS, threshold=0.1, max_passes=5, dilate=0)
    whole = tp.run(**par)
    tiles = [tp.run(rows=np.arange(a, min(a + 5, ms.H)), **par) for a in range(0, ms.H, 5)]
    assert np.array_equal(np.concatenate([t.moments for t in tiles]), whole.moments)
    assert np.array_equal(np.concatenate([t.passes for t in tiles]), whole.passes)
    par["dilate"] = 1   # ... and with it they need not: the neighbourhood is the call's
    tiled = np.concatenate([tp.run(rows=np.arange(a, min(a + 5, ms.H)), **par).passes for a in range(0, ms.H, 5)])
    assert tiled.shape == whole.passes.shape


# ---- the cases beyond one selection block ---------------------------------------------------------------------------------------------

SELECT_BLOCK = 1024            # flux_amd/csrc/adaptive.hip kSelectBlock: the pixels adaptive_select_kernel compacts per block
COUNT_BLOCK, COUNT_BLOCKS = 256, 64   # ... kBlock and launch_adaptive_count's largest grid: beyond their product the count kernel strides
# name -> (rounds, active pixels per selection block and round (None: too many to list), pass histogram (None: not pinned)), measured
# on the reference alone
BLOCK_FIGURES = {
    "blocks-41x27-2": (6, [[1024, 83], [411, 38], [302, 24], [305, 0], [307, 0], [304, 0]], {1: 618, 2: 146, 3: 35, 4: 18, 5: 29, 6: 261}),
    "blocks-67x47-3": (4, [[1024, 1024, 1024, 77], [450, 500, 475, 25], [403, 452, 366, 21], [403, 463, 376, 21]], None),
    "blocks-130x127-2": (3, None, {1: 11097, 2: 1187, 3: 4226}),
}
STRIDED_ROWS = np.arange(1, 47, 2)    # of blocks-67x47-3: tests/test_gpu_adaptive.py's strided device call
TILE_ROWS = 10                        # ... and its row tiles, with dilate 1


def test_the_block_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "flux_amd", "csrc", "adaptive.hip")).read()
    assert f"constexpr unsigned kSelectBlock = {SELECT_BLOCK}," in src and f"constexpr unsigned kBlock = {COUNT_BLOCK};" in src
    assert f"blocks < {COUNT_BLOCKS} ? blocks : {COUNT_BLOCKS}" in src


@pytest.mark.parametrize("name", list(asp.BLOCK_CASES))
def test_block_case_conditions(flux, name):
    """test_gpu_case_conditions' margins for the frames of more than one selection block, and what each frame is there to reach."""
    _, par, res = asp.case(flux, name)
    w, h = asp.BLOCK_CASES[name][3]
    rounds, per_block, hist = BLOCK_FIGURES[name]
    blocks, waves = asp.block_counts(res, SELECT_BLOCK), asp.block_waves(res, SELECT_BLOCK)
    got_hist = {int(c): int(k) for c, k in zip(*np.unique(res.passes, return_counts=True))}
    print(f"adaptive case {name}: {w * h} pixels, rounds {len(res.active)}, pass histogram {got_hist}, decision margin "
          f"{res.decision_margin:.2e}, path margin {res.path_margin:.2e}; active pixels per block and round "
          f"{blocks if len(blocks[0]) <= 4 else [sum(b) for b in blocks]}")
    assert res.decision_margin >= 1e-9
    assert res.path_margin >= ms.MIN_MARGIN
    assert res.passes.shape == (h, w) and len(res.active) == rounds
    assert len(blocks[0]) == -(-w * h // SELECT_BLOCK) > 1
    if per_block is not None:
        assert blocks == per_block
    if hist is not None:
        assert got_hist == hist
    assert any(16 in wv for wv in waves[1:])   # a selection (rounds >= 1) with a block whose 16 waves all hold an active pixel
    assert np.isfinite(res.moments).all()
    assert w % 16 and w % 7                    # no width is a multiple of the pixels a wave holds (16 at root 2, 7 at root 3)
    if name == "blocks-41x27-2":
        assert all(wv[0] == 16 for wv in waves)   # ... here the first block, in every round
    if name == "blocks-130x127-2":
        assert w * h > COUNT_BLOCKS * COUNT_BLOCK and len(blocks[0]) == 17


def test_some_round_has_an_empty_selection_block_beside_a_non_empty_one(flux):
    found = [(name, r) for name in asp.BLOCK_CASES for r, b in enumerate(asp.block_counts(asp.case(flux, name)[2], SELECT_BLOCK))
             if r >= 1 and 0 in b and any(b)]
    assert ("blocks-41x27-2", 3) in found and ("blocks-41x27-2", 5) in found, found


def test_strided_rows_and_row_tiles_have_a_neighbourhood_of_their_own(flux):
    """What the GPU suite's strided and tiled calls with dilation rest on: the rule over rows 1, 3, ... 45 of the 67 x 47 frame
    (dilate 2) and over its tiles of 10 rows (dilate 1) keeps the margins, fills two selection blocks, and gives ANOTHER pass map
    than the frame's run does on those rows -- a kernel that dilates in global rows cannot pass both."""
    _, par, whole = asp.case(flux, "blocks-67x47-3")
    _, _, sub = asp.rows_case(flux, "blocks-67x47-3", STRIDED_ROWS)
    differ = int(np.count_nonzero(sub.passes != whole.passes[STRIDED_ROWS]))
    blocks = asp.block_counts(sub, SELECT_BLOCK)
    print(f"adaptive strided rows of blocks-67x47-3: {sub.passes.size} pixels, active per block and round {blocks}, pass map differs from "
          f"the frame's rows in {differ} pixels; decision margin {sub.decision_margin:.2e}, path margin {sub.path_margin:.2e}")
    assert sub.passes.size == 1541 and blocks == [[1024, 517], [470, 244], [415, 176], [422, 184]]
    assert differ == 200
    assert sub.decision_margin >= 1e-9 and sub.path_margin >= ms.MIN_MARGIN
    _, par1, whole1 = asp.rows_case(flux, "blocks-67x47-3", np.arange(47), dilate=1)
    assert par1["dilate"] == 1 and whole1.decision_margin >= 1e-9
    tiles = [asp.rows_case(flux, "blocks-67x47-3", np.arange(a, min(a + TILE_ROWS, 47)), dilate=1)[2] for a in range(0, 47, TILE_ROWS)]
    for t in tiles:
        assert t.decision_margin >= 1e-9 and t.path_margin >= ms.MIN_MARGIN
    tiled = np.concatenate([t.passes for t in tiles])
    differ1 = int(np.count_nonzero(tiled != whole1.passes))
    print(f"adaptive tiles of {TILE_ROWS} rows of blocks-67x47-3, dilate 1: pass map differs from the frame's in {differ1} pixels")
    assert tiled.shape == whole1.passes.shape and differ1 > 0
    assert [t.passes.shape[0] for t in tiles] == [10, 10, 10, 10, 7]


def test_the_comparison_for_non_finite_references(flux):
    """moments_spec.assert_close_where_finite and adaptive_spec's: assert_close on a finite reference; with a NaN and an inf in the
    reference they demand them in the same places, and the bounds elsewhere."""
    _, want, rad, _, _ = ms.reference(flux, "open", 2)
    got = want.copy()
    got[..., ms.S2] *= 1.0 + 4e-10
    assert ms.group_errors(got, want, ms.mean_lum(rad) ** 2, 4.0, ms.max_to_one_factor(want)) == ms.errors(got, want, rad)
    ms.assert_close_where_finite(got, want, rad, "finite")
    poisoned = want.copy()
    poisoned[2, 3, :], poisoned[5, 6, 4], poisoned[5, 6, 0] = np.nan, np.inf, np.nan
    got = poisoned.copy()
    got[5, 6, 4] = np.nan     # (another non-finite value in the same place: the mask is what is compared)
    ms.assert_close_where_finite(got, poisoned, rad, "poisoned")
    for y, x, ch, v in ((2, 3, 1, 0.5), (0, 0, 7, np.nan), (5, 6, 0, 0.0), (1, 1, 5, want[1, 1, 5] + 1e-8), (4, 4, 7, want[4, 4, 7] * 1.001 + 1e-8)):
        bad = poisoned.copy()
        bad[y, x, ch] = v
        with pytest.raises(AssertionError):
            ms.assert_close_where_finite(bad, poisoned, rad, "bad")
    _, par, res = asp.case(flux, "open-2")
    asp.assert_close_where_finite(res.moments, res.passes, res, "finite", 4)
    bad = res.moments.copy()
    bad[3, 3, 7] = bad[3, 3, 7] * 1.001 + 1e-8
    with pytest.raises(AssertionError):
        asp.assert_close_where_finite(bad, res.passes, res, "bad", 4)
    with pytest.raises(AssertionError):
        asp.assert_close_where_finite(res.moments, res.passes + np.uint32(1), res, "bad", 4)


# ---- the quality table of DESIGN.md section 5h ----------------------------------------------------------------------------------------

# scene -> the bound asserted on relMSE(adaptive) / relMSE(uniform), the measured ratio plus 10 %; None: adaptive is NOT better there
# and nothing is asserted.  Measured at the defaults with max_passes 16: demo2 58.57 spp against uniform 64 spp, ratio 1.823 (2715 of
# the 3072 pixels run into the 16-pass limit, and sixteen independent sets of 4 samples lack the stratification of one set of 64);
# demo1 29.15 spp against uniform 36 spp, ratio 0.985.
QUALITY = {"demo2": None, "demo1": 0.985 * 1.1}
_quality = {}


def rel_mse(x, ref, lum_floor):
    return float(np.mean((np.asarray(x) - ref) ** 2 / (ref ** 2 + lum_floor ** 2)))


def quality(flux, oracle_mod, name):
    """One row of the table: 64 x 48, root 2, seed 7, depth 5, the defaults with max_passes 16, against the restatement at sample
    root 40, seed 11; the uniform frame at the smallest root whose root² is at least the adaptive mean samples per pixel."""
    if name not in _quality:
        sd = small_scene(flux.load_scene(os.path.join(SCENES, name + ".yml")), 64, 48)
        ref = oracle_mod.Oracle(sd, flux.JobConfiguration(40, 5, 50), seed=11).render_frame(threads=min(16, os.cpu_count() or 1))
        par = dict(asp.DEFAULTS, max_passes=16)
        base = PathSpec(sd, 2, 5, 7)
        try:
            res = asp.TracedPasses(base).run(**par)
            base.frame()
            aov = aov_buffers(base)
        finally:
            base.close()
        spp = 4.0 * float(res.passes.mean())
        root = int(np.ceil(np.sqrt(spp)))
        uni = PathSpec(sd, root, 5, 7)
        try:
            frame = uni.frame()
            umom = ms.from_samples(uni.sample_radiance)
        finally:
            uni.close()
        floor = par["lum_floor"]
        ad = res.moments[..., ms.RGB]
        _quality[name] = dict(spp=spp, root=root, mse=(denoise_spec.mse(ad, ref), denoise_spec.mse(frame, ref)),
                              rel=(rel_mse(ad, ref, floor), rel_mse(frame, ref, floor)),
                              den=(denoise_spec.mse(dms.denoise_moments(res.moments, aov), ref),
                                   denoise_spec.mse(dms.denoise_moments(umom, aov), ref)),
                              rounds=len(res.active), full=int((res.passes == 16).sum()))
    return _quality[name]


@pytest.mark.parametrize("name", list(QUALITY))
def test_quality_against_a_converged_render(flux, oracle_mod, name):
    q = quality(flux, oracle_mod, name)
    print(f"adaptive quality {name}: {q['spp']:.2f} samples per pixel in {q['rounds']} rounds ({q['full']} pixels at 16 passes) against uniform "
          f"root {q['root']} ({q['root'] ** 2} spp): MSE {q['mse'][0]:.3e} / {q['mse'][1]:.3e} = {q['mse'][0] / q['mse'][1]:.3f}, relative MSE "
          f"{q['rel'][0]:.3e} / {q['rel'][1]:.3e} = {q['rel'][0] / q['rel'][1]:.3f}, after denoise_moments MSE {q['den'][0]:.3e} / {q['den'][1]:.3e} "
          f"= {q['den'][0] / q['den'][1]:.3f}")
    assert q["root"] ** 2 >= q["spp"]  # the uniform frame never has fewer samples
    if QUALITY[name] is not None:
        assert q["rel"][0] < QUALITY[name] * q["rel"][1]


# ---- the entry points' argument checks: before any device call ------------------------------------------------------------------------

BAD_PARAMS = [
    (dict(threshold=float("nan")), "threshold"), (dict(threshold=float("inf")), "threshold"), (dict(threshold=-0.1), "threshold"),
    (dict(lum_floor=float("nan")), "lum_floor"), (dict(lum_floor=float("inf")), "lum_floor"), (dict(lum_floor=0.0), "lum_floor"),
    (dict(lum_floor=-1.0), "lum_floor"), (dict(min_passes=0), "min_passes must be"), (dict(min_passes=3, max_passes=2), "below min_passes"),
    (dict(dilate=3), "dilate"), (dict(reserved=1), "reserved"),
]


def _params(L, **over):
    v = dict(threshold=0.05, lum_floor=0.01, min_passes=1, max_passes=8, dilate=1, reserved=0)
    v.update(over)
    return L.FluxAdaptiveParams(v["threshold"], v["lum_floor"], v["min_passes"], v["max_passes"], v["dilate"], v["reserved"])


def test_both_entry_points_refuse_bad_arguments_without_a_device(flux):
    """Each refusal by its own message; a context is not even looked at before the parameters pass (0x1000 is never dereferenced).
    The refusals that need a context -- a set-share context, sample_root 1, max_passes > S, rows, stride, null outputs -- are in
    tests/test_gpu_adaptive.py."""
    L = flux._lib
    lib = L.lib
    mom, passes = np.zeros((2, 3, 8)), np.zeros((2, 3), dtype=np.uint32)
    pm, pp = mom.ctypes.data_as(C.POINTER(C.c_double)), passes.ctypes.data_as(C.c_void_p)
    for over, word in BAD_PARAMS:
        par = _params(L, **over)
        for ctx in (None, 0x1000):
            assert lib.flux_render_adaptive_rows(ctx, 0, 1, C.byref(par), pm, pp, None) == L.E_INVALID, over
            assert word in L.last_error() and "flux_render_adaptive_rows:" in L.last_error(), L.last_error()
            assert lib.flux_render_adaptive_rows_device(ctx, 0, 1, 2, C.byref(par), 0x2000, 0x3000, None, None) == L.E_INVALID, over
            assert word in L.last_error() and "flux_render_adaptive_rows_device:" in L.last_error(), L.last_error()
    messages = set()
    for over, _ in BAD_PARAMS:
        lib.flux_render_adaptive_rows(None, 0, 1, C.byref(_params(L, **over)), pm, pp, None)
        messages.add(L.last_error().split(":", 1)[1].strip().split(" ")[0])
    assert len(messages) == 6, messages  # a message of its own for each rule (the seventh, max_passes > S, needs a context)
    good = _params(L)
    assert lib.flux_render_adaptive_rows(None, 0, 1, None, pm, pp, None) == L.E_INVALID and "null params" in L.last_error()
    assert lib.flux_render_adaptive_rows_device(None, 0, 1, 2, None, 0x2000, 0x3000, None, None) == L.E_INVALID and "null params" in L.last_error()
    assert lib.flux_render_adaptive_rows(None, 0, 1, C.byref(good), pm, pp, None) == L.E_INVALID and "null context" in L.last_error()
    assert lib.flux_render_adaptive_rows_device(None, 0, 1, 2, C.byref(good), 0x2000, 0x3000, None, None) == L.E_INVALID
    assert "null context" in L.last_error()
    assert np.all(mom == 0.0) and np.all(passes == 0)


def test_python_names(flux):
    L = flux._lib
    for name in ("ADAPTIVE_THRESHOLD", "ADAPTIVE_LUM_FLOOR", "ADAPTIVE_MIN_PASSES", "ADAPTIVE_MAX_PASSES", "ADAPTIVE_DILATE"):
        assert name in flux.__all__ and hasattr(flux, name)
    for name in ("render_adaptive", "render_adaptive_device", "last_adaptive_info"):
        assert hasattr(flux.Renderer, name)
    for name in ("flux_render_adaptive_rows", "flux_render_adaptive_rows_device"):
        assert name in L.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "flux_abi.h")).read()
    for line in (f"#define FLUX_ADAPTIVE_THRESHOLD {flux.ADAPTIVE_THRESHOLD}", f"#define FLUX_ADAPTIVE_LUM_FLOOR {flux.ADAPTIVE_LUM_FLOOR}",
                 f"#define FLUX_ADAPTIVE_MIN_PASSES {flux.ADAPTIVE_MIN_PASSES}", f"#define FLUX_ADAPTIVE_MAX_PASSES {flux.ADAPTIVE_MAX_PASSES}",
                 f"#define FLUX_ADAPTIVE_DILATE {flux.ADAPTIVE_DILATE}", f"#define FLUX_ADAPTIVE_INFO_WORDS {L.ADAPTIVE_INFO_WORDS}",
                 "#define FLUX_ABI_VERSION 3"):
        assert line in hdr, line
    assert asp.DEFAULTS == dict(threshold=flux.ADAPTIVE_THRESHOLD, lum_floor=flux.ADAPTIVE_LUM_FLOOR, min_passes=flux.ADAPTIVE_MIN_PASSES,
                                max_passes=flux.ADAPTIVE_MAX_PASSES, dilate=flux.ADAPTIVE_DILATE)
    # the ctypes mirror has the header's layout: two doubles, four 32-bit words
    assert C.sizeof(L.FluxAdaptiveParams) == 32
    assert [(n, getattr(L.FluxAdaptiveParams, n).offset) for n, _ in L.FluxAdaptiveParams._fields_] == [
        ("threshold", 0), ("lum_floor", 8), ("min_passes", 16), ("max_passes", 20), ("dilate", 24), ("reserved", 28)]
    body = hdr[hdr.index("typedef struct flux_adaptive_params {"):hdr.index("} flux_adaptive_params;")]
    order = [body.index(f" {n};") for n, _ in L.FluxAdaptiveParams._fields_]
    assert order == sorted(order)
    with pytest.raises(flux.FluxError, match="bad row range"):  # never reaches the library
        flux.Renderer.render_adaptive(flux.Renderer.__new__(flux.Renderer), row_start=2, row_end=1)
    assert "denoise_moments" in flux.Renderer.render_adaptive.__doc__


# ---- flux_host::render_adaptive and its helpers ------------------------------------------------------------------------------------

def test_cpp_adaptive_helpers_check_their_buffers(tmp_path):
    exe = selftest.build(str(tmp_path / "adaptive_host_selftest"), "adaptive_host_selftest.cpp", host=True, compiler="g++")
    out = selftest.run(exe)
    assert "all ok" in out


def test_cpp_adaptive_helpers_under_sanitizers(tmp_path):
    """The same program as a stand-alone sanitized executable: the host layer it calls is compiled into it with
    -fsanitize=address,undefined.  It is about host code, so it is shown no device: the valid call ends in FLUX_E_DEVICE everywhere."""
    exe = selftest.build(str(tmp_path / "adaptive_host_selftest_san"), "adaptive_host_selftest.cpp", host=True, flags=selftest.SANITIZE,
                         compiler="g++")
    assert "all ok" in selftest.run(exe, env=selftest.sanitize_env(HIP_VISIBLE_DEVICES="-1"))


# ---- the command-line tool --------------------------------------------------------------------------------------------------------------

def test_flux_help_names_the_flags():
    flux_bin, _ = host_bins()
    out = subprocess.run([flux_bin, "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    assert "--adaptive <THRESHOLD>" in out.stderr + out.stdout and "--adaptive-max-passes" in out.stderr + out.stdout


def test_flux_adaptive_flags_are_refused_with_status_2_before_any_job(tmp_path):
    flux_bin, _ = host_bins()
    scene = os.path.join(SCENES, "demo2.yml")
    for args, word in ((["--adaptive-max-passes", "4"], "needs that flag"), (["--adaptive", "much"], "much"), (["--adaptive", "-0.5"], "-0.5"),
                       (["--adaptive", "nan"], "nan"), (["--adaptive", "inf"], "inf"), (["--adaptive"], "requires a value"),
                       (["--adaptive", "0.05", "--adaptive-max-passes", "0"], "--adaptive-max-passes"),
                       (["--adaptive", "0.05", "--adaptive-max-passes", "x"], "--adaptive-max-passes"),
                       (["--adaptive", "0.05", "--adaptive-max-passes"], "requires a value")):
        out = subprocess.run([flux_bin, scene, "--outdir", str(tmp_path), *args], capture_output=True, text=True, timeout=60)
        assert out.returncode == 2, (args, out.returncode, out.stderr)
        assert "--adaptive" in out.stderr and word in out.stderr, out.stderr
        assert "Rendering" not in out.stdout and "Connecting" not in out.stdout
    # with good values the flags are accepted: what refuses the run here is the missing local GPU, as for --aov
    for extra in ([], ["--adaptive-max-passes", "4"]):
        out = subprocess.run([flux_bin, scene, "--adaptive", "0.05", *extra, "--gpus", "0", "--outdir", str(tmp_path)],
                             capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and "local GPU" in out.stderr and "--adaptive" in out.stderr, out.stderr
    assert os.listdir(tmp_path) == []
