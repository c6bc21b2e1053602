"""The feature-guided a-trous filter of flux_denoise (include/flux_abi.h) restated in numpy: the
specification the kernels of flux_amd/csrc/denoise.hip are held against (tests/test_denoise.py, tests/test_gpu_denoise.py).

Every sum and product is written in the order the header states it: taps run rows outer (j), columns inner (i); a skipped tap
adds an exact 0.0, which leaves a running sum's bits alone.  The one function the kernels evaluate differently is exp2 (fexp2 of
flux_math.h, <= 2 ulp from np.exp2)."""
import numpy as np

H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])
DEFAULTS = dict(levels=5, sigma_l=2.0, sigma_n=0.35, sigma_z=0.1, sigma_a=0.1)
E_MAX = 1100.0   # exponents are clamped here: 2^-1100 is 0 in f64
SD_FLOOR = 1e-8  # added to sigma_l * sqrt(var)


def lum(c):
    return (0.2126 * c[..., 0] + 0.7152 * c[..., 1]) + 0.0722 * c[..., 2]


def norm2(v):
    return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


def max_to_one(x):
    """Color::max_to_one (color.rs:35-44)."""
    m = np.maximum(np.maximum(x[..., 0], x[..., 1]), x[..., 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(m > 1.0, 1.0 / m, 1.0)
    return np.where((m > 1.0)[..., None], x * s[..., None], x)


def usable(rgb, aov):
    """Every component of rgb, albedo and normal finite, the luminance finite, the depth not NaN (+inf is a depth)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.isfinite(rgb).all(axis=2) & np.isfinite(aov[..., 0:6]).all(axis=2) & np.isfinite(lum(rgb))
                & ~np.isnan(aov[..., 6]))


def _shifted(arrays, dy, dx, h, w):
    """The arrays read at (y + dy, x + dx), and which of those reads lie on the image (the others hold a clamped pixel)."""
    ys, xs = np.arange(h) + dy, np.arange(w) + dx
    on = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]
    yy, xx = np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1)
    return [a[yy][:, xx] for a in arrays], on


def guide(a, n, z, aq, nq, zq, sn2, sz2, sa2):
    """G(p, q) with sn2 = sigma_n * sigma_n and so on."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        en = norm2(n - nq) / sn2
        d = (z - zq) / ((np.abs(z) + np.abs(zq)) + 1e-300)
        ez = np.where(np.isfinite(z) & np.isfinite(zq), (d * d) / sz2, np.where(z == zq, 0.0, np.inf))
        ea = norm2(a - aq) / sa2
        return (en + ez) + ea


def filter_levels(rgb, aov, ok, variance, levels, sigma_l, sigma_n, sigma_z, sigma_a):
    """The filter over the frame `rgb`, given which pixels are usable and where the variance comes from that the first level starts
    from: variance(c, taps) with c the frame, unusable pixels zeroed, and taps(x) the walk over the step-1 taps, rows outer, that
    yields (valid, wt, xq) per tap -- whether a pixel may use it, its weight from the guides alone (0 where it may not) and x read
    at the tap."""
    h, w, _ = rgb.shape
    assert aov.shape == (h, w, 8) and 1 <= levels <= 8
    a, n, z = aov[..., 0:3], aov[..., 3:6], aov[..., 6]
    sn2, sz2, sa2 = sigma_n * sigma_n, sigma_z * sigma_z, sigma_a * sigma_a
    c = np.where(ok[..., None], rgb, 0.0)
    zero = np.zeros((h, w))

    def taps(x):
        for j in range(-2, 3):
            for i in range(-2, 3):
                (xq, aq, nq, zq, okq), on = _shifted([x, a, n, z, ok], j, i, h, w)
                valid = on & okq & ok
                yield valid, np.where(valid, np.exp2(-np.minimum(guide(a, n, z, aq, nq, zq, sn2, sz2, sa2), E_MAX)), 0.0), xq

    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        var = np.where(ok, variance(c, taps), 0.0)
        for k in range(levels):
            s = 1 << k
            sd = sigma_l * np.sqrt(var) + SD_FLOOR
            l = lum(c)
            num, den, vnum = np.zeros_like(c), zero.copy(), zero.copy()
            for j in range(-2, 3):
                for i in range(-2, 3):
                    (cq, lq, vq, aq, nq, zq, okq), on = _shifted([c, l, var, a, n, z, ok], j * s, i * s, h, w)
                    valid = on & okq & ok
                    e = np.minimum(guide(a, n, z, aq, nq, zq, sn2, sz2, sa2) + np.abs(l - lq) / sd, E_MAX)
                    wt = np.where(valid, (H5[j + 2] * H5[i + 2]) * np.exp2(-e), 0.0)
                    num += np.where(valid[..., None], wt[..., None] * cq, 0.0)
                    den += wt
                    vnum += np.where(valid, (wt * wt) * vq, 0.0)
            c = np.where(ok[..., None], num / den[..., None], 0.0)
            var = np.where(ok, vnum / (den * den), 0.0)
    out = max_to_one(c)
    out[~ok] = rgb[~ok]  # bit for bit
    return out


def denoise(rgb, aov, levels=5, sigma_l=2.0, sigma_n=0.35, sigma_z=0.1, sigma_a=0.1):
    rgb = np.array(rgb, dtype=np.float64)
    aov = np.asarray(aov, dtype=np.float64)
    ok = usable(rgb, aov)

    def variance(c, taps):
        """Of the luminance over the 5 x 5 neighbourhood, weighted by the guides alone: two passes."""
        seen, s0, s1 = [], np.zeros(ok.shape), np.zeros(ok.shape)
        for valid, wt, lq in taps(lum(c)):
            s0 += wt
            s1 += np.where(valid, wt * lq, 0.0)
            seen.append((valid, wt, lq))
        m = np.where(ok, s1 / s0, 0.0)
        s2 = np.zeros(ok.shape)
        for valid, wt, lq in seen:
            d = lq - m
            s2 += np.where(valid, wt * (d * d), 0.0)
        return s2 / s0

    return filter_levels(rgb, aov, ok, variance, levels, sigma_l, sigma_n, sigma_z, sigma_a)


def synthetic(h, w, seed=3):
    """Random colour over two guide regions (a normal + depth edge at w // 2), a row of +inf depth, a NaN pixel, a pixel with one
    inf channel, a NaN normal and a black albedo -- each placed only where the image has room for it."""
    rng = np.random.default_rng(seed)
    rgb = rng.random((h, w, 3)) * 1.2
    aov = np.zeros((h, w, 8))
    aov[..., 0:3] = 0.5 + 0.02 * rng.random((h, w, 3))
    aov[..., 3:6] = (0.0, 1.0, 0.0)
    aov[..., 6] = 5.0 + 0.05 * rng.random((h, w))
    aov[..., 7] = 1.0
    if w >= 2:
        aov[:, w // 2:, 3:6] = (1.0, 0.0, 0.0)
        aov[:, w // 2:, 6] += 4.0
    if h >= 2:
        aov[0, :, 6] = np.inf
    if h >= 8 and w >= 8:
        aov[3, 3, 0:3] = 0.0
        rgb[5, 5] = np.nan
        rgb[6, w - 4, 1] = np.inf
        aov[7, 2, 4] = np.nan
        aov[2, 6, 6] = np.nan
    elif h * w >= 6:
        rgb.reshape(-1, 3)[h * w - 1] = np.nan
        rgb.reshape(-1, 3)[h * w - 2, 2] = np.inf
    return rgb, aov


def mse(x, ref):
    return float(np.nanmean((x - ref) ** 2))
