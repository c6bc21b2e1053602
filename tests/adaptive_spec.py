"""Adaptive sampling (include/flux_abi.h flux_render_adaptive_rows) as numpy: the reference the tests hold the kernels
against, built on tests/path_spec.py -- `Oracle.primary_ray(row, col, set, i)` and `PathSpec._trace(o, d, sets, idx)` take an
arbitrary sample set, so pass c of a pixel is traced with set (set0 + c) % W -- and the test cases with the conditions they meet.

The rule, for a call over `rows` (h of them, W columns), N = sample_root², S = W:
    state    per pixel the running sums of r, g, b, l, l² and a pass count c, all 0
    rounds   r = 0, 1, ... while r < max_passes; in rounds r < min_passes every pixel is active; afterwards, per pixel,
                 n = N c, m = Σl / n, s² = max(0, Σl² - (Σl Σl) / n) / (n - 1), e² = (s² / n) / max(m, lum_floor)²
             hot iff e² > τ² (never for a NaN), active iff a hot pixel lies within Chebyshev distance `dilate` in the call's local
             row and column index, clipped at the call's edges; stop at the first round with no active pixel
    a pass   of an active pixel: the N samples of set (set0 + c) % S summed in index order into five totals, each total added to its
             running sum with one addition, c += 1
    output   moments_spec's eight channels with n = N c for N, and the map of c
The kernel adds a pass's samples up per lane and then over lanes, so its sums differ from these by rounding."""
import atexit

import numpy as np

import moments_spec as ms
from conftest import small_scene
from path_spec import PathSpec

DEFAULTS = dict(threshold=0.05, lum_floor=0.01, min_passes=1, max_passes=8, dilate=1)  # include/flux_abi.h FLUX_ADAPTIVE_*


class Result:
    """moments [h, w, 8]; passes [h, w] uint32; active: per round run the [h, w] mask of the pixels that took a pass; hot: per
    selection made the [h, w] mask (hot[k] decided round min_passes + k); decision_margin: the smallest |e² - τ²| / (τ² + 1 / n) over
    every hot decision taken (NaN decisions aside); sums [h, w, 5]: the state; path_margin (TracedPasses.run): PathSpec's smallest
    decision margin over every pass traced for the scene so far."""


def dilated(hot, dilate):
    """active[y, x] = any hot within Chebyshev distance `dilate`, clipped at the array's edges."""
    h, w = hot.shape
    out = np.zeros_like(hot)
    for dy in range(-dilate, dilate + 1):
        for dx in range(-dilate, dilate + 1):
            ys, yd = slice(max(dy, 0), h + min(dy, 0)), slice(max(-dy, 0), h + min(-dy, 0))
            xs, xd = slice(max(dx, 0), w + min(dx, 0)), slice(max(-dx, 0), w + min(-dx, 0))
            out[yd, xd] |= hot[ys, xs]
    return out


def error2(sl, sl2, c, N, lum_floor):
    """e² per pixel from the running sums (c >= 1 everywhere)."""
    with np.errstate(all="ignore"):
        n = (N * c).astype(np.float64)
        m = sl / n
        d = sl2 - (sl * sl) / n
        s2 = np.where(d < 0.0, 0.0, d) / (n - 1.0)
        mm = np.where(m > lum_floor, m, lum_floor)
        return (s2 / n) / (mm * mm)


def finish(sums, c, N):
    """[h, w, 5] running sums and the pass map -> moments_spec's eight channels with n = N c."""
    with np.errstate(all="ignore"):
        n = (N * c).astype(np.float64)
        mean = sums[..., 0:3] * (1.0 / n)[..., None]
        mx1 = np.where(mean[..., 0] > mean[..., 1], mean[..., 0], mean[..., 1])
        mx2 = np.where(mx1 > mean[..., 2], mx1, mean[..., 2])
        k = np.where(mx2 > 1.0, 1.0 / mx2, 1.0)
        rgb = np.where((mx2 > 1.0)[..., None], mean * k[..., None], mean)
        d = sums[..., 4] - (sums[..., 3] * sums[..., 3]) / n
        s2 = np.where(d < 0.0, 0.0, d) / (n - 1.0)
        out = np.empty(c.shape + (ms.CHANNELS,))
        out[..., ms.RGB], out[..., ms.VAR], out[..., ms.MEAN], out[..., ms.S2] = rgb, (s2 / n) * (k * k), mean, s2
    return out


def adaptive(sampler, h, w, N, threshold, max_passes, min_passes=1, lum_floor=0.01, dilate=1):
    """The rule over any source of samples: sampler(ys, xs, cs) -> [k, N, 3], the radiance of pass cs[j] of local pixel
    (ys[j], xs[j])."""
    assert N >= 4 and 1 <= min_passes <= max_passes and 0 <= dilate <= 2 and threshold >= 0.0 and lum_floor > 0.0
    sums, c = np.zeros((h, w, 5)), np.zeros((h, w), dtype=np.int64)
    res = Result()
    res.active, res.hot, res.decision_margin = [], [], np.inf
    tau2 = threshold * threshold
    for r in range(max_passes):
        if r < min_passes:
            active = np.ones((h, w), bool)
        else:
            e2 = error2(sums[..., 3], sums[..., 4], c, N, lum_floor)
            with np.errstate(all="ignore"):
                hot = e2 > tau2
                margin = np.abs(e2 - tau2) / (tau2 + 1.0 / (N * c))
            margin = margin[np.isfinite(margin)]
            if margin.size:
                res.decision_margin = min(res.decision_margin, float(margin.min()))
            res.hot.append(hot)
            active = dilated(hot, dilate)
            if not active.any():
                break
        ys, xs = np.nonzero(active)
        rad = np.asarray(sampler(ys, xs, c[ys, xs]), dtype=np.float64)
        assert rad.shape == (len(ys), N, 3)
        with np.errstate(all="ignore"):
            tot, tl, tl2 = np.zeros((len(ys), 3)), np.zeros(len(ys)), np.zeros(len(ys))
            for i in range(N):  # moments_spec.from_samples' order
                tot = tot + rad[:, i]
                l = ms.lum(rad[:, i])
                tl = tl + l
                tl2 = tl2 + l * l
            sums[ys, xs, 0:3] = sums[ys, xs, 0:3] + tot
            sums[ys, xs, 3] = sums[ys, xs, 3] + tl
            sums[ys, xs, 4] = sums[ys, xs, 4] + tl2
        c[ys, xs] += 1
        res.active.append(active)
    res.moments, res.passes, res.sums = finish(sums, c, N), c.astype(np.uint32), sums
    return res


class TracedPasses:
    """The passes of a PathSpec's scene, traced on demand and kept: pass c of pixel (row, col) always reads set (set0 + c) % W, so
    its radiance is shared by every run over the scene, whatever the parameters and however rows are grouped."""

    def __init__(self, spec: PathSpec):
        self.spec, self.N, self.W = spec, spec.N, spec.width
        self._rad = {}      # (row, col, c) -> [N, 3]
        self._set0 = {}     # row -> [W]
        self.path_margin = np.inf

    def set0(self, row):
        if row not in self._set0:
            self._set0[row] = np.asarray(self.spec._oracle.row_perm(row)).astype(np.int64) % self.W
        return self._set0[row]

    def passes(self, rows, cols, cs):
        """[k, N, 3] for global pixels (rows[j], cols[j]) at pass cs[j]."""
        need = [(int(r), int(x), int(c)) for r, x, c in zip(rows, cols, cs) if (int(r), int(x), int(c)) not in self._rad]
        if need:
            N = self.N
            o, d = np.empty((len(need) * N, 3)), np.empty((len(need) * N, 3))
            sets = np.empty(len(need) * N, dtype=int)
            for j, (r, x, c) in enumerate(need):
                s = int((self.set0(r)[x] + c) % self.W)
                sets[j * N:(j + 1) * N] = s
                for i in range(N):
                    o[j * N + i], d[j * N + i] = self.spec._oracle.primary_ray(r, x, s, i)
            rad, _, margins, _, _ = self.spec._trace(o, d, sets, np.tile(np.arange(N), len(need)))
            self.path_margin = min(self.path_margin, min(margins.values()))
            for j, key in enumerate(need):
                self._rad[key] = rad[j * N:(j + 1) * N].copy()
        return np.stack([self._rad[(int(r), int(x), int(c))] for r, x, c in zip(rows, cols, cs)]) if len(rows) else np.zeros((0, self.N, 3))

    def run(self, rows=None, **params):
        """The rule over the global `rows` (default: the frame) of the scene; adds path_margin to the result."""
        rows = np.arange(self.spec.height) if rows is None else np.asarray(rows)
        res = adaptive(lambda ys, xs, cs: self.passes(rows[ys], xs, cs), len(rows), self.W, self.N, **params)
        res.path_margin = self.path_margin
        return res


def errors(got, want, passes, N):
    """The largest error per channel group against moments_spec's bounds with n = N c for N: channels 0-2 and 4-6 absolute;
    channel 7 relative to (ref + m²), channel 3 relative to (ref + m² k² / n), m the mean luminance."""
    n = N * passes.astype(np.float64)
    m2 = ms.lum(want[..., ms.MEAN]) ** 2
    mx = want[..., ms.MEAN].max(axis=2)
    k = np.where(mx > 1.0, 1.0 / np.maximum(mx, 1.0), 1.0)
    diff = np.abs(np.asarray(got) - want)

    def rel(d, den):
        with np.errstate(all="ignore"):
            return float(np.where(den > 0.0, d / den, np.where(d == 0.0, 0.0, np.inf)).max())
    return {"rgb": float(diff[..., ms.RGB].max()), "mean": float(diff[..., ms.MEAN].max()),
            "var": rel(diff[..., ms.VAR], want[..., ms.VAR] + m2 * k * k / n), "s2": rel(diff[..., ms.S2], want[..., ms.S2] + m2)}


def assert_close(got, got_passes, want, label, N):
    """The pass map equal; 1e-9 absolute on channels 0-2 and 4-6, 1e-9 (ref + scale) on channels 3 and 7; prints the figures first."""
    assert got.shape == want.moments.shape and got_passes.shape == want.passes.shape
    differ = int(np.count_nonzero(got_passes != want.passes))
    print(f"adaptive {label}: pass maps differ in {differ} pixels")
    assert differ == 0, label
    err = errors(got, want.moments, want.passes, N)
    print(f"adaptive {label}: max error rgb {err['rgb']:.2e} mean {err['mean']:.2e} (absolute), var {err['var']:.2e} s2 {err['s2']:.2e} "
          f"(relative to ref + scale)")
    assert np.isfinite(got).all(), label
    assert all(e <= ms.TOL for e in err.values()), (label, err)


# ---- the cases of the GPU suite (tests/test_gpu_adaptive.py), 16 x 12 frames: S = 16 ---------------------------------------------------
# name -> (scene, sample_root, parameters).  τ is picked per case so that the conditions of tests/test_adaptive.py hold: decision
# margin >= 1e-9, path margin >= 1e-10, a pass map that is not constant, a pixel that stops early, one that reaches max_passes, one
# active only through dilation.
CASES = {
    "open-2": ("open", 2, dict(threshold=0.2, max_passes=6, dilate=1)),
    "open-3": ("open", 3, dict(threshold=0.15, max_passes=5, dilate=1)),
    "open-8": ("open", 8, dict(threshold=0.05, max_passes=3, dilate=1)),
    "open-10": ("open", 10, dict(threshold=0.04, max_passes=3, dilate=1)),
    "open_mesh-8": ("open_mesh", 8, dict(threshold=0.05, max_passes=3, dilate=1)),
    "glass-4": ("glass", 4, dict(threshold=0.24, max_passes=4, dilate=1)),
    "box_room-4": ("box_room", 4, dict(threshold=0.8, max_passes=4, dilate=1)),
    "disk_light-4": ("disk_light", 4, dict(threshold=0.12, max_passes=4, dilate=1)),
    "wrap-2": ("open", 2, dict(threshold=0.1, max_passes=16, dilate=2)),  # sets wrap past S = 16
}
# ... and two that cannot meet those conditions by what they are: a 3 x 2 frame (S = 3) whose last list has ONE entry, and a frame
# whose first selection finds nothing hot, so that the call stops in round 1 with c = 1 everywhere.  name -> (..., (w, h)).
SPECIAL = {
    "single-3x2": ("open", 2, dict(threshold=0.5, max_passes=3, dilate=0), (3, 2)),
    "round1-2": ("open", 2, dict(threshold=1.2, max_passes=6, dilate=1), (ms.W, ms.H)),
}
# ... and three frames of more than one selection block (adaptive.hip kSelectBlock = 1024 pixels), scene `open` at other sizes.  At 192
# pixels adaptive_select_kernel is one block of three waves and adaptive_count_kernel never strides; here a block's base comes from
# another block's atomic add, an empty block sits beside a non-empty one, and the 130 x 127 frame is more than the 64 x 256 pixels
# the count kernel covers without striding.  tests/test_adaptive.py asserts what each reaches from the reference alone.
BLOCK_CASES = {
    "blocks-41x27-2": ("open", 2, dict(threshold=0.2, max_passes=6, dilate=1), (41, 27)),
    "blocks-67x47-3": ("open", 3, dict(threshold=0.15, max_passes=4, dilate=2), (67, 47)),
    "blocks-130x127-2": ("open", 2, dict(threshold=0.2, max_passes=3, dilate=1), (130, 127)),
}
DEPTH, SEED = ms.DEPTH, ms.SEED
_traced = {}
_runs = {}
_row_runs = {}


@atexit.register
def _close():  # (the restatement's contexts, while its library is still loaded)
    for tp in _traced.values():
        tp.spec.close()
    _traced.clear()


def traced(flux, scene_name, root, w=ms.W, h=ms.H):
    """The TracedPasses of a scene and sample root, one per process (its PathSpec stays open)."""
    key = (scene_name, root, w, h)
    if key not in _traced:
        sd = ms.scene(flux, scene_name, w, h)
        if (sd.output_settings.image_width, sd.output_settings.image_height) != (w, h):
            sd = small_scene(sd, w, h)
        _traced[key] = TracedPasses(PathSpec(sd, root, DEPTH, SEED))
    return _traced[key]


def case(flux, name):
    """(scene, parameters with the defaults filled in, Result) of a case, computed once and shared, read-only."""
    if name not in _runs:
        scene_name, root, par, size = CASES[name] + ((ms.W, ms.H),) if name in CASES else SPECIAL.get(name) or BLOCK_CASES[name]
        par = dict(DEFAULTS, **par)
        tp = traced(flux, scene_name, root, *size)
        res = tp.run(**par)
        res.moments.setflags(write=False)
        res.passes.setflags(write=False)
        _runs[name] = (tp.spec.sd, par, res)
    return _runs[name]


def counts(res, par):
    """(pixels that stop early, pixels at max_passes, pixel-rounds active only through dilation, distinct pass counts)."""
    only_dilated = 0
    for k, hot in enumerate(res.hot):
        r = par["min_passes"] + k
        if r < len(res.active):
            only_dilated += int(np.count_nonzero(res.active[r] & ~hot))
    return (int(np.count_nonzero(res.passes < par["max_passes"])), int(np.count_nonzero(res.passes == par["max_passes"])),
            only_dilated, len(np.unique(res.passes)))


def rows_case(flux, name, rows, **over):
    """(scene, parameters, Result) of a case's rule run over the global `rows` alone -- the neighbourhood is the call's --, the
    parameters of the case with `over` on top; computed once and shared, read-only."""
    key = (name, tuple(int(r) for r in rows), tuple(sorted(over.items())))
    if key not in _row_runs:
        sd, par, _ = case(flux, name)
        scene_name, root, _, size = BLOCK_CASES[name]
        par = dict(par, **over)
        res = traced(flux, scene_name, root, *size).run(rows=np.asarray(rows), **par)
        res.moments.setflags(write=False)
        res.passes.setflags(write=False)
        _row_runs[key] = (sd, par, res)
    return _row_runs[key]


def block_counts(res, block):
    """Per round, the active pixels in each run of `block` consecutive pixels of the call (row-major: the selection's blocks)."""
    return [[int(a.ravel()[b:b + block].sum()) for b in range(0, a.size, block)] for a in res.active]


def block_waves(res, block, wave=64):
    """Per round and block, the number of the block's `wave`-pixel runs that hold an active pixel."""
    return [[sum(bool(a.ravel()[w:min(w + wave, b + block)].any()) for w in range(b, min(b + block, a.size), wave))
             for b in range(0, a.size, block)] for a in res.active]


def assert_close_where_finite(got, got_passes, want, label, N):
    """assert_close for a reference that may hold non-finite values (moments_spec.assert_close_where_finite): the pass map equal,
    the same finite mask per channel, the bounds wherever the reference is finite."""
    assert got.shape == want.moments.shape and got_passes.shape == want.passes.shape
    differ = int(np.count_nonzero(got_passes != want.passes))
    print(f"adaptive {label}: pass maps differ in {differ} pixels")
    assert differ == 0, label
    with np.errstate(all="ignore"):
        err = ms.group_errors(got, want.moments, ms.lum(want.moments[..., ms.MEAN]) ** 2, N * want.passes.astype(np.float64),
                              ms.max_to_one_factor(want.moments))
    odd = int(np.count_nonzero(~np.isfinite(want.moments)))
    print(f"adaptive {label}: max error rgb {err['rgb']:.2e} mean {err['mean']:.2e} (absolute), var {err['var']:.2e} s2 {err['s2']:.2e} "
          f"(relative to ref + scale) where the reference is finite; {odd} non-finite values in it")
    for ch in range(ms.CHANNELS):
        assert np.array_equal(np.isfinite(got[..., ch]), np.isfinite(want.moments[..., ch])), (label, "finite mask of channel", ch)
    assert all(e <= ms.TOL for e in err.values()), (label, err)
