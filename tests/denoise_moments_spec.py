"""flux_denoise_moments (include/flux_abi.h) restated in numpy: the filter of tests/denoise_spec.py with exactly two
changes -- a usable pixel must also have a finite variance v >= 0, and the variance a level starts from is the MEASURED one,
prefiltered over the step-1 taps with the guide weights, var_p = sum w v_q / sum w in one pass, instead of the spatial estimate.
`prefilter=False` skips the prefilter (var_p = v_p): not an entry point of the library, only the middle column of §5g's table."""
import numpy as np

from denoise_spec import E_MAX, H5, SD_FLOOR, _shifted, guide, lum, max_to_one, usable


def usable_moments(rgb, v, aov):
    with np.errstate(invalid="ignore"):
        return usable(rgb, aov) & np.isfinite(v) & (v >= 0.0)


def denoise_moments(moments, aov, levels=5, sigma_l=2.0, sigma_n=0.35, sigma_z=0.1, sigma_a=0.1, prefilter=True):
    moments = np.asarray(moments, dtype=np.float64)
    aov = np.asarray(aov, dtype=np.float64)
    rgb, v = np.array(moments[..., 0:3]), moments[..., 3]
    h, w, _ = rgb.shape
    assert moments.shape == (h, w, 8) and aov.shape == (h, w, 8) and 1 <= levels <= 8
    ok = usable_moments(rgb, v, aov)
    a, n, z = aov[..., 0:3], aov[..., 3:6], aov[..., 6]
    sn2, sz2, sa2 = sigma_n * sigma_n, sigma_z * sigma_z, sigma_a * sigma_a
    c = np.where(ok[..., None], rgb, 0.0)
    v = np.where(ok, v, 0.0)
    zero = np.zeros((h, w))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if prefilter:
            s0, s1 = zero.copy(), zero.copy()
            for j in range(-2, 3):
                for i in range(-2, 3):
                    (vq, aq, nq, zq, okq), on = _shifted([v, a, n, z, ok], j, i, h, w)
                    valid = on & okq & ok
                    wt = np.where(valid, np.exp2(-np.minimum(guide(a, n, z, aq, nq, zq, sn2, sz2, sa2), E_MAX)), 0.0)
                    s0 += wt
                    s1 += np.where(valid, wt * vq, 0.0)
            var = np.where(ok, s1 / s0, 0.0)
        else:
            var = v
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
