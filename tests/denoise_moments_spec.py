"""flux_denoise_moments (include/flux_abi.h) restated in numpy: the filter of tests/denoise_spec.py with exactly two
changes -- a usable pixel must also have a finite variance v >= 0, and the variance a level starts from is the MEASURED one,
prefiltered over the step-1 taps with the guide weights, var_p = sum w v_q / sum w in one pass, instead of the spatial estimate.
`prefilter=False` skips the prefilter (var_p = v_p): not an entry point of the library, only the middle column of §5g's table."""
import numpy as np

from denoise_spec import filter_levels, usable


def usable_moments(rgb, v, aov):
    with np.errstate(invalid="ignore"):
        return usable(rgb, aov) & np.isfinite(v) & (v >= 0.0)


def denoise_moments(moments, aov, levels=5, sigma_l=2.0, sigma_n=0.35, sigma_z=0.1, sigma_a=0.1, prefilter=True):
    moments = np.asarray(moments, dtype=np.float64)
    aov = np.asarray(aov, dtype=np.float64)
    assert moments.ndim == 3 and moments.shape[2] == 8
    rgb, v = np.array(moments[..., 0:3]), moments[..., 3]
    ok = usable_moments(rgb, v, aov)
    v = np.where(ok, v, 0.0)

    def variance(c, taps):
        if not prefilter:
            return v
        s0, s1 = np.zeros(ok.shape), np.zeros(ok.shape)
        for valid, wt, vq in taps(v):
            s0 += wt
            s1 += np.where(valid, wt * vq, 0.0)
        return s1 / s0

    return filter_levels(rgb, aov, ok, variance, levels, sigma_l, sigma_n, sigma_z, sigma_a)


def synthetic(h, w, seed=3):
    """denoise_spec.synthetic's frame and guides as a moments buffer with a random v, and -- where the image has room -- a zero, a
    NaN, a negative and an inf entry in v."""
    from denoise_spec import synthetic as base
    rgb, aov = base(h, w, seed)
    rng = np.random.default_rng(seed + 100)
    mom = np.zeros((h, w, 8))
    mom[..., 0:3] = rgb
    mom[..., 3] = 0.02 * rng.random((h, w)) ** 2
    mom[..., 4:7] = rgb
    mom[..., 7] = mom[..., 3] * 4.0
    flat = mom.reshape(-1, 8)
    if h * w >= 6:
        flat[0, 3] = 0.0
    if h >= 8 and w >= 8:
        mom[4, 9, 3] = np.nan
        mom[9, 4, 3] = -1e-3
        mom[10, 12, 3] = np.inf
        mom[8, 8, 3] = 0.0
    elif h * w >= 6:
        flat[1, 3] = np.nan
        flat[2, 3] = -1.0
        flat[3, 3] = np.inf
    return mom, aov
