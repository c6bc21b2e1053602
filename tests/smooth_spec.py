"""Smooth meshes (include/flux_abi.h flux_ctx_set_mesh_normals) in numpy: the call's checks and normalisation, the
barycentrics of a hit recomputed with the hit test's own expressions, and the interpolated shading normal with its fall-back to the
facet normal.  Plain IEEE f64 in the order the header states; no GPU.  Works on one hit (vectors [3]) or on rows ([m, 3])."""
import numpy as np

L2_MIN = 1e-24  # below it -- and for a NaN -- the facet normal stands


def _dot(a, b):
    """(x x' + y y') + z z', on single vectors or on rows"""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def check_normals(corners):
    """The call's refusal for corner normals [nt, 3, 3]: None, or (triangle, corner) of the first normal that is not finite with a
    finite length > 0."""
    c = np.asarray(corners, dtype=np.float64).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        nn = _dot(c, c)
        bad = ~(np.isfinite(c).all(axis=-1) & np.isfinite(nn) & (nn > 0.0))
    if bad.any():
        k, j = np.argwhere(bad)[0]
        return int(k), int(j)
    return None


def normalize(corners):
    """n / sqrt(n.n) per corner, [nt, 3, 3]"""
    c = np.asarray(corners, dtype=np.float64).reshape(-1, 3, 3)
    return c / np.sqrt(_dot(c, c))[..., None]


def facet_normal(v0, e1, e2):
    """normalize(e1 x e2) as the host build stores it; zeros for a triangle without area"""
    nn = _cross(np.asarray(e1, dtype=np.float64), np.asarray(e2, dtype=np.float64))
    with np.errstate(all="ignore"):
        length = np.sqrt(_dot(nn, nn))
        return np.where((length > 0.0)[..., None], nn / length[..., None], 0.0)


def barycentrics(v0, e1, e2, o, d):
    """(u, v) of the segment (o, d) on the triangle (v0, e1, e2): p = d x e2, inv = 1 / (e1.p), s = o - v0, u = (s.p) inv,
    q = s x e1, v = (d.q) inv -- Moeller-Trumbore's expressions, as the hit test has them."""
    v0, e1, e2, o, d = (np.asarray(x, dtype=np.float64) for x in (v0, e1, e2, o, d))
    with np.errstate(all="ignore"):
        p = _cross(d, e2)
        inv = 1.0 / _dot(e1, p)
        s = o - v0
        u = _dot(s, p) * inv
        q = _cross(s, e1)
        v = _dot(d, q) * inv
    return u, v


def interpolate(u, v, n0, n1, n2, facet):
    """(shading normal, l2): w = (1 - u) - v, m = (w n0 + u n1) + v n2, l2 = (m.x^2 + m.y^2) + m.z^2; m / sqrt(l2) where
    l2 >= 1e-24, the facet normal elsewhere (a NaN fails the comparison)."""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    n0, n1, n2, facet = (np.asarray(x, dtype=np.float64) for x in (n0, n1, n2, facet))
    with np.errstate(all="ignore"):
        w = (1.0 - u) - v
        m = (w[..., None] * n0 + u[..., None] * n1) + v[..., None] * n2
        l2 = (m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]) + m[..., 2] * m[..., 2]
        ok = l2 >= L2_MIN
        n = np.where(ok[..., None], m / np.sqrt(np.where(ok, l2, 1.0))[..., None], np.broadcast_to(facet, m.shape))
    return n, l2


def shading_normal(v0, e1, e2, corners, o, d, facet=None):
    """The shading normal of the hit of (o, d) on the triangle (v0, e1, e2) with NORMALISED corner normals `corners` [..., 3, 3]."""
    corners = np.asarray(corners, dtype=np.float64)
    if facet is None:
        facet = facet_normal(v0, e1, e2)
    u, v = barycentrics(v0, e1, e2, o, d)
    return interpolate(u, v, corners[..., 0, :], corners[..., 1, :], corners[..., 2, :], facet)[0]


def mesh_triangles(mesh):
    """(v0, e1, e2, facet) [nt, 3] each of a MeshData, with the host build's operations: e1 = v1 - v0, e2 = v2 - v0; a triangle whose
    e1 x e2 is exactly zero has its edges cleared and a zero normal."""
    v = np.asarray(mesh.vertices, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(mesh.triangles, dtype=np.int64).reshape(-1, 3)
    v0, e1, e2 = v[t[:, 0]], v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]
    facet = facet_normal(v0, e1, e2)
    dead = ~(_cross(e1, e2) != 0.0).any(axis=-1)
    e1, e2 = np.where(dead[:, None], 0.0, e1), np.where(dead[:, None], 0.0, e2)
    return v0, e1, e2, facet
