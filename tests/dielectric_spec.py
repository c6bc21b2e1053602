"""The Dielectric bounce (include/flux_abi.h FLUX_MAT_DIELECTRIC) stated in numpy, operation for operation in the
order the spec writes it -- the order the STRICT kernels evaluate it in.  Shared by tests/test_dielectric_scene.py (its self-checks)
and tests/test_gpu_dielectric.py (rays against the kernels)."""
import numpy as np


def fresnel(n, d, ri):
    """Per ray: (F, c, eta, m, ct, dh) for shading normals n [k,3], directions d [k,3] and refraction index ri."""
    n = np.asarray(n, dtype=np.float64)
    d = np.asarray(d, dtype=np.float64)
    ln = np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
    ld = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    nh = n / ln[:, None]
    dh = d / ld[:, None]
    c = -(dh[:, 0] * nh[:, 0] + dh[:, 1] * nh[:, 1] + dh[:, 2] * nh[:, 2])
    outside = c > 0.0
    eta = np.where(outside, ri, 1.0 / ri)
    m = np.where(outside[:, None], nh, -nh)
    c = np.where(outside, c, -c)
    with np.errstate(invalid="ignore", divide="ignore"):
        k = 1.0 - (1.0 - c * c) / (eta * eta)
        tir = k < 0.0
        ct = np.where(tir, 0.0, np.sqrt(np.where(tir, 0.0, k)))
        rs = (c - eta * ct) / (c + eta * ct)
        rp = (eta * c - ct) / (eta * c + ct)
        F = np.where(tir, 1.0, (rs * rs + rp * rp) / 2.0)
    return F, c, eta, m, ct, dh


def bounce(n, d, ri, u):
    """Per ray: (reflect [k] bool, wi [k,3], F [k]) -- u <= F reflects."""
    F, c, eta, m, ct, dh = fresnel(n, d, ri)
    refl = np.asarray(u) <= F
    c2 = 2.0 * c
    wr = dh + c2[:, None] * m
    a = c / eta - ct
    wt = dh / eta[:, None] + a[:, None] * m
    return refl, np.where(refl[:, None], wr, wt), F


def fresnel_cos(cos_i, ri):
    """F for a ray arriving from the outside at incidence cosine cos_i (the spec's formula on scalars / arrays)."""
    c = np.asarray(cos_i, dtype=np.float64)
    eta = ri
    with np.errstate(invalid="ignore"):
        k = 1.0 - (1.0 - c * c) / (eta * eta)
        ct = np.sqrt(np.maximum(k, 0.0))
        rs = (c - eta * ct) / (c + eta * ct)
        rp = (eta * c - ct) / (eta * c + ct)
    return np.where(k < 0.0, 1.0, (rs * rs + rp * rp) / 2.0)
