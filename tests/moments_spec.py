"""The per-pixel sample moments (include/flux_abi.h flux_render_moments_rows) as numpy: the reference the tests hold
the kernel against, built from the per-sample radiance of tests/path_spec.py, and the test scenes with the conditions they must meet.

For a pixel with samples L_0 .. L_{N-1} (N = sample_root², in index order) and l_i = (0.2126 L_i.r + 0.7152 L_i.g) + 0.0722 L_i.b:
    mean  = (sum L_i) * (1 / N)                                   channels 4-6, unclamped
    rgb   = max_to_one(mean)                                      channels 0-2: PathSpec.frame() bit for bit
    s2    = max(0, sum l_i² - (sum l_i)² / N) / (N - 1)           channel 7 (one pass; the max keeps a NaN)
    var   = (s2 / N) * k²,  k = 1 / max(mean) where that is > 1   channel 3: the variance of lum(rgb)
The kernel adds the samples up per lane and then over lanes, so its sums differ from these by rounding."""
import os

import numpy as np

import aov_spec
from conftest import SCENES, small_scene
from path_spec import PathSpec

CHANNELS = 8
RGB, VAR, MEAN, S2 = slice(0, 3), 3, slice(4, 7), 7
SEED, DEPTH = 7, 5
W, H = aov_spec.W, aov_spec.H
TOL = 1e-9

# scene, sample_root -> (noisy pixels: s2 / N > 1e-3 m², zero-variance pixels: numpy's two-pass variance of the luminance is exactly
# 0 -- the one-pass s2 of such a pixel is 0 or at rounding level --, clamped pixels: max(mean) > 1) of the 192, counted on the CPU
# from PathSpec's samples.  They keep the comparison with the kernel from being blind: an N for N - 1 slip
# moves every noisy pixel by >= 1 %, the zero-variance pixels are what the denoiser's prefilter is for, and k != 1 only where clamped.
CASES = {
    ("open", 2): (116, 65, 25), ("open", 3): (122, 59, 23), ("open", 8): (71, 54, 23), ("open", 10): (62, 16, 23),
    ("open_mesh", 8): (71, 29, 23), ("glass", 4): (172, 0, 27), ("box_room", 4): (126, 66, 4), ("disk_light", 4): (161, 0, 10),
    ("demo2", 4): (169, 0, 27), ("demo1", 4): (94, 79, 0),
}
MIN_MARGIN = 1e-10  # no decision of any sample sits at rounding level (the smallest, `open` root 10: 5.6e-10)


def lum(c):
    return (0.2126 * c[..., 0] + 0.7152 * c[..., 1]) + 0.0722 * c[..., 2]


def from_samples(rad):
    """[H, W, N, 3] per-sample radiance -> [H, W, 8]."""
    rad = np.asarray(rad, dtype=np.float64)
    h, w, N, _ = rad.shape
    assert N >= 2
    with np.errstate(all="ignore"):
        s, sl, sl2 = np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w))
        for i in range(N):
            s = s + rad[:, :, i]
            l = lum(rad[:, :, i])
            sl = sl + l
            sl2 = sl2 + l * l
        mean = s * (1.0 / float(N))
        mx1 = np.where(mean[..., 0] > mean[..., 1], mean[..., 0], mean[..., 1])
        mx2 = np.where(mx1 > mean[..., 2], mx1, mean[..., 2])
        k = np.where(mx2 > 1.0, 1.0 / mx2, 1.0)
        rgb = np.where((mx2 > 1.0)[..., None], mean * k[..., None], mean)
        d = sl2 - (sl * sl) / float(N)
        s2 = np.where(d < 0.0, 0.0, d) / (float(N) - 1.0)
        out = np.empty((h, w, CHANNELS))
        out[..., RGB], out[..., VAR], out[..., MEAN], out[..., S2] = rgb, (s2 / float(N)) * (k * k), mean, s2
    return out


def two_pass_s2(rad):
    """numpy's two-pass sample variance of the luminance, [H, W]."""
    return np.var(lum(np.asarray(rad, dtype=np.float64)), axis=2, ddof=1)


def mean_lum(rad):
    return lum(np.asarray(rad, dtype=np.float64)).mean(axis=2)


def counts(mom, rad):
    """(noisy, zero-variance, clamped) pixels."""
    N = rad.shape[2]
    m = mean_lum(rad)
    return (int(np.count_nonzero(mom[..., S2] / N > 1e-3 * m * m)), int(np.count_nonzero(two_pass_s2(rad) == 0.0)),
            int(np.count_nonzero(mom[..., MEAN].max(axis=2) > 1.0)))


def scene(flux, name, w=W, h=H):
    if name == "open":
        return aov_spec.open_scene(flux)
    if name == "open_mesh":
        return aov_spec.open_mesh_scene(flux)
    return small_scene(flux.load_scene(os.path.join(SCENES, name + ".yml")), w, h)


_refs = {}


def reference(flux, name, root, w=W, h=H, seed=SEED):
    """(scene, moments [H, W, 8], per-sample radiance [H, W, N, 3], PathSpec.frame(), smallest decision margin), computed once per
    case and shared, read-only."""
    key = (name, root, w, h, seed)
    if key not in _refs:
        sd = scene(flux, name, w, h)
        spec = PathSpec(sd, root, DEPTH, seed)
        try:
            frame = spec.frame()
            rad, margin = spec.sample_radiance, spec.min_margin()
        finally:
            spec.close()
        mom = from_samples(rad)
        for a in (mom, rad, frame):
            a.setflags(write=False)
        _refs[key] = (sd, mom, rad, frame, margin)
    return _refs[key]


def errors(got, want, rad):
    """The largest error per channel group against its bound: channels 0-2 and 4-6 absolute; channel 7 relative to (ref + m²),
    channel 3 relative to (ref + m² k² / N)."""
    N = rad.shape[2]
    m2 = mean_lum(rad) ** 2
    mx = want[..., MEAN].max(axis=2)
    k = np.where(mx > 1.0, 1.0 / np.maximum(mx, 1.0), 1.0)
    diff = np.abs(np.asarray(got) - want)

    def rel(d, den):  # (a black pixel has ref + scale = 0: an equal value is no error there, any other an infinite one)
        with np.errstate(all="ignore"):
            return float(np.where(den > 0.0, d / den, np.where(d == 0.0, 0.0, np.inf)).max())
    return {"rgb": float(diff[..., RGB].max()), "mean": float(diff[..., MEAN].max()),
            "var": rel(diff[..., VAR], want[..., VAR] + m2 * k * k / N), "s2": rel(diff[..., S2], want[..., S2] + m2)}


def assert_close(got, want, rad, label):
    """1e-9 absolute on channels 0-2 and 4-6, 1e-9 (ref + scale) on channels 3 and 7; prints the figures first."""
    assert got.shape == want.shape
    err = errors(got, want, rad)
    print(f"moments {label}: max error rgb {err['rgb']:.2e} mean {err['mean']:.2e} (absolute), var {err['var']:.2e} s2 {err['s2']:.2e} "
          f"(relative to ref + scale)")
    assert np.isfinite(got).all(), label
    assert all(e <= TOL for e in err.values()), (label, err)


def group_errors(got, want, m2, n, k):
    """errors()' four figures over the entries where `want` is finite, for references that hold a NaN or an inf (a scene whose
    normals are not unit vectors).  m2: the squared mean luminance [H, W]; n: the sample count, a number or [H, W]; k: max_to_one's
    factor [H, W].  Where the reference is finite and ref + scale is not a positive number, only an equal value is no error."""
    finite = np.isfinite(want)
    with np.errstate(all="ignore"):
        diff = np.where(finite, np.abs(np.asarray(got) - want), 0.0)

        def rel(ch, scale):
            den = want[..., ch] + scale
            e = np.where(den > 0.0, diff[..., ch] / den, np.where(diff[..., ch] == 0.0, 0.0, np.inf))
            return float(np.where(finite[..., ch], e, 0.0).max())
        return {"rgb": float(diff[..., RGB].max()), "mean": float(diff[..., MEAN].max()), "var": rel(VAR, m2 * k * k / n), "s2": rel(S2, m2)}


def max_to_one_factor(want):
    with np.errstate(all="ignore"):
        mx = want[..., MEAN].max(axis=2)
        return np.where(mx > 1.0, 1.0 / np.maximum(mx, 1.0), 1.0)


def assert_close_where_finite(got, want, rad, label):
    """assert_close for a reference that may hold non-finite values: the SAME finite mask in each of the eight channels, and
    assert_close's bounds wherever the reference is finite; prints the figures first.  On a finite reference it is assert_close."""
    assert got.shape == want.shape
    with np.errstate(all="ignore"):
        err = group_errors(got, want, mean_lum(rad) ** 2, float(rad.shape[2]), max_to_one_factor(want))
    odd = int(np.count_nonzero(~np.isfinite(want)))
    print(f"moments {label}: max error rgb {err['rgb']:.2e} mean {err['mean']:.2e} (absolute), var {err['var']:.2e} s2 {err['s2']:.2e} "
          f"(relative to ref + scale) where the reference is finite; {odd} non-finite values in it")
    for ch in range(CHANNELS):
        assert np.array_equal(np.isfinite(got[..., ch]), np.isfinite(want[..., ch])), (label, "finite mask of channel", ch)
    assert all(e <= TOL for e in err.values()), (label, err)
