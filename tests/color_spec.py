"""Vertex colours (include/flux_abi.h flux_ctx_set_mesh_colors) in numpy: the call's checks and its rounding to f32,
and the colour factor of a hit -- the corner colours interpolated at smooth_spec's barycentrics and clamped below at 0.  Plain IEEE
f64 in the order the header states; no GPU.  Works on one hit (vectors [3]) or on rows ([m, 3])."""
import numpy as np

import smooth_spec

FLT_MAX = float(np.finfo(np.float32).max)


def check_colors(corners):
    """The call's refusal for corner colours [nt, 3, 3]: None, or (triangle, corner, channel) of the first component x that does not
    satisfy x >= 0 and x <= FLT_MAX (a NaN fails both)."""
    c = np.asarray(corners, dtype=np.float64).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        bad = ~((c >= 0.0) & (c <= FLT_MAX))
    if bad.any():
        k, j, ch = np.argwhere(bad)[0]
        return int(k), int(j), int(ch)
    return None


def store(corners):
    """(float)x per component, round-to-nearest-even: the stored corner colours k0, k1, k2 as float32 [nt, 3, 3]"""
    return np.asarray(corners, dtype=np.float64).reshape(-1, 3, 3).astype(np.float32)


def interpolate(u, v, k0, k1, k2):
    """The colour factor c [..., 3] at barycentrics (u, v) of stored (f32) corner colours: per channel, with k* widened to f64,
    g1 = k1 - k0, g2 = k2 - k0, c = (k0 + u g1) + v g2, c = fmax(c, 0.0) -- IEEE maxNum: a NaN gives 0."""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    k0, k1, k2 = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (k0, k1, k2))
    with np.errstate(all="ignore"):
        g1 = k1 - k0
        g2 = k2 - k0
        c = (k0 + u[..., None] * g1) + v[..., None] * g2
        return np.fmax(c, 0.0)


def color_factor(v0, e1, e2, stored, o, d):
    """c of the hit of the segment (o, d) on the triangle (v0, e1, e2) with STORED corner colours `stored` [..., 3, 3]"""
    stored = np.asarray(stored)
    u, v = smooth_spec.barycentrics(v0, e1, e2, o, d)
    return interpolate(u, v, stored[..., 0, :], stored[..., 1, :], stored[..., 2, :])
