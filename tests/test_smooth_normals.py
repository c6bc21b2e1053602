"""Smooth meshes without a GPU: the numpy statement of the rule (tests/smooth_spec.py) against its own
properties, the loader and the procedural meshes, the entry point's checks that need no device, and the host half of the call
(flux_amd/csrc/flux_mesh_attr.h) as a stand-alone program, plain and under the sanitizers."""
import os

import numpy as np
import pytest

import mesh_attr_checks as checks
import smooth_spec
from conftest import SCENES


def _ulp_distance(a, b):
    return np.max(np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b))))


def _random_triangles(rng, m):
    v0 = rng.uniform(-3, 3, (m, 3))
    e1, e2 = rng.uniform(-2, 2, (m, 3)), rng.uniform(-2, 2, (m, 3))
    corners = smooth_spec.normalize(rng.normal(size=(m, 3, 3)))
    return v0, e1, e2, corners


# ---- the spec -----------------------------------------------------------------------------------------------------------------

def test_a_vertex_gets_its_own_normal():
    rng = np.random.default_rng(1)
    v0, e1, e2, corners = _random_triangles(rng, 50)
    facet = smooth_spec.facet_normal(v0, e1, e2)
    for k, (u, v) in enumerate(((0.0, 0.0), (1.0, 0.0), (0.0, 1.0))):
        n, l2 = smooth_spec.interpolate(np.full(50, u), np.full(50, v), corners[:, 0], corners[:, 1], corners[:, 2], facet)
        # the weights are exactly 1, 0, 0: m is the corner itself and m / sqrt(m.m) one normalisation of a unit vector
        assert _ulp_distance(n, corners[:, k]) <= 2.0
        assert np.all(np.abs(l2 - 1.0) < 1e-15)


def test_three_equal_corner_normals_return_that_normal():
    rng = np.random.default_rng(2)
    n0 = smooth_spec.normalize(rng.normal(size=(400, 3, 3)))[:, 0]
    u = rng.uniform(0, 1, 400)
    v = rng.uniform(0, 1, 400) * (1.0 - u)
    n, _ = smooth_spec.interpolate(u, v, n0, n0, n0, np.zeros(3))
    big = np.abs(n0) > 0.05   # (an ulp of a tiny component is not the scale of the sum's rounding)
    assert _ulp_distance(n[big], n0[big]) <= 2.0
    assert np.max(np.abs(n - n0)) <= 4 * 2.220446049250313e-16


def test_opposed_normals_fall_back_to_the_facet_normal():
    up, facet = np.array([0.0, 1.0, 0.0]), np.array([0.6, 0.0, 0.8])
    n, l2 = smooth_spec.interpolate(0.5, 0.0, up, -up, up, facet)   # midpoint of the edge v0 v1: m = 0
    assert l2 == 0.0 and np.array_equal(n, facet)
    n, l2 = smooth_spec.interpolate(0.5 + 1e-13, 0.0, up, -up, up, facet)   # l2 = 4e-26 < 1e-24
    assert 0.0 < l2 < smooth_spec.L2_MIN and np.array_equal(n, facet)
    n, l2 = smooth_spec.interpolate(0.5 + 1e-11, 0.0, up, -up, up, facet)   # l2 = 4e-22: interpolated
    assert l2 > smooth_spec.L2_MIN and np.array_equal(n, -up)


def test_a_nan_never_leaves_it():
    facet = np.array([0.0, 0.0, 1.0])
    tri = (np.zeros(3), np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]))
    corners = smooth_spec.normalize(np.array([[[0, 0, 1.0], [0, 1.0, 1.0], [1.0, 0, 1.0]]]))[0]
    cases = [(np.array([0.2, 0.2, 1.0]), np.array([1.0, 0.0, 0.0])),       # a ray in the triangle's plane: e1.p = 0, inv = inf, 0 inf = NaN
             (np.array([np.nan, 0.2, 1.0]), np.array([0.0, 0.0, -1.0])),   # a NaN origin
             (np.array([0.2, 0.2, 1.0]), np.array([0.0, 0.0, -np.inf])),   # an infinite direction
             (np.array([1e308, 1e308, 1.0]), np.array([0.0, 0.0, -1.0]))]  # barycentrics that overflow
    for o, d in cases:
        n = smooth_spec.shading_normal(*tri, corners, o, d, facet)
        assert np.all(np.isfinite(n)), (o, d, n)
        assert np.array_equal(n, facet) or abs(float(n @ n) - 1.0) < 1e-15
    assert np.array_equal(smooth_spec.shading_normal(*tri, corners, *cases[0], facet), facet)
    nan_corners = corners.copy()
    nan_corners[1, 1] = np.nan   # (the call refuses such a table; the rule itself still holds)
    n = smooth_spec.shading_normal(*tri, nan_corners, np.array([0.2, 0.2, 1.0]), np.array([0.0, 0.0, -1.0]), facet)
    assert np.array_equal(n, facet)


def _moller_trumbore(v0, e1, e2, o, d):
    """numpy's own: cross products by np.cross, dots by einsum, the division written as one"""
    p = np.cross(d, e2)
    det = np.einsum("ij,ij->i", e1, p)
    s = o - v0
    u = np.einsum("ij,ij->i", s, p) / det
    v = np.einsum("ij,ij->i", d, np.cross(s, e1)) / det
    t = np.einsum("ij,ij->i", e2, np.cross(s, e1)) / det
    return u, v, t


def test_barycentrics_equal_a_numpy_moller_trumbore_on_random_hits():
    rng = np.random.default_rng(3)
    v0, e1, e2, _ = _random_triangles(rng, 2000)
    bu = rng.uniform(0, 1, 2000)
    bv = rng.uniform(0, 1, 2000) * (1.0 - bu)
    target = v0 + bu[:, None] * e1 + bv[:, None] * e2
    o = target + rng.normal(size=(2000, 3)) * 3.0
    d = target - o
    u, v = smooth_spec.barycentrics(v0, e1, e2, o, d)
    mu, mv, mt = _moller_trumbore(v0, e1, e2, o, d)
    # the same quantities in another association (a product with the reciprocal against a division): a few ulp of values of
    # order 1, conditioned by |e1| |p| / |e1.p| -- the sample keeps well-conditioned triangles
    area = np.linalg.norm(np.cross(e1, e2), axis=1)
    good = (area > 0.5) & (np.abs(np.einsum("ij,ij->i", e1, np.cross(d, e2))) > 0.5)
    assert good.sum() > 1000
    assert np.max(np.abs(u - mu)[good]) < 1e-12 and np.max(np.abs(v - mv)[good]) < 1e-12
    assert np.max(np.abs(u - bu)[good]) < 1e-11 and np.max(np.abs(v - bv)[good]) < 1e-11
    assert np.all(np.abs(mt[good] - 1.0) < 1e-11)


# ---- the loader, the procedural meshes ------------------------------------------------------------------------------------------

_load = checks.load


def test_normals_round_trip_into_the_calls_layout(flux):
    from flux_amd.scene import corner_normals
    per_vertex = [[0, 0, -1], [0.5, 0, -1], [0.5, 0.5, -2], [0, 0.25, -1]]
    sd = _load(flux, f"normals: {per_vertex}")
    mesh = sd.shapes[0]
    assert mesh.normals.shape == (4, 3) and mesh.normals.dtype == np.float64
    c = corner_normals(mesh)
    assert c.shape == (2, 3, 3) and c.flags["C_CONTIGUOUS"] and c.dtype == np.float64
    want = np.array(per_vertex, dtype=np.float64)[np.array([[0, 1, 2], [0, 2, 3]])]
    assert np.array_equal(c, want)   # not normalised here: the library does that
    # per corner: taken as given
    import dataclasses
    per_corner = np.arange(18, dtype=np.float64).reshape(2, 3, 3) + 1.0
    assert np.array_equal(corner_normals(dataclasses.replace(mesh, normals=per_corner)), per_corner)
    # absent: None, and a Triangle stays flat
    assert _load(flux, "").shapes[0].normals is None and corner_normals(_load(flux, "").shapes[0]) is None
    tri = flux.scene.shape_from_yaml({"Triangle": {"v0": [0, 0, 0], "v1": [1, 0, 0], "v2": [0, 1, 0], "normals": [[0, 0, 1]] * 3,
                                                   "material": {"Emissive": {"color": [1, 1, 1], "power": 1.0}}}})
    assert tri.normals is None


@pytest.mark.parametrize("line,message", [
    ("normals: [[0, 0, 1], [0, 0, 1], [0, 0, 1]]", "expected one [x,y,z] per vertex (4), got 3"),
    ("normals: 7", "expected one [x,y,z] per vertex (4)"),
    ("normals: [[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, x, 1]]", "normals[3]: expected a sequence of 3 numbers"),
    ("normals: [[0, 0, 1], [0, 0, 1], [0, 0], [0, 0, 1]]", "normals[2]: expected a sequence of 3 numbers"),
    ("normals: [[0, 0, 1], [0, 0, 0], [0, 0, 1], [0, 0, 1]]", "triangle 0, corner 1: normal (0.0, 0.0, 0.0) must be finite"),
    ("normals: [[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, .inf, 1]]", "triangle 1, corner 2"),
    ("normals: [[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, .nan, 1]]", "triangle 1, corner 2"),
])
def test_loader_refusals(flux, line, message):
    checks.loader_refusal(flux, line, message)


def test_meshdata_refusals(flux):
    checks.meshdata_refusals(flux, "normals", np.full((4, 3), 1e200), "triangle 0, corner 0")   # a length that overflows


def test_procedural_meshes(flux):
    from flux_amd.procedural import heightfield_mesh, uv_sphere_mesh, vertex_normals
    ball = uv_sphere_mesh(8, 6, (1.0, 2.0, 3.0), 0.5)
    v, t = ball.vertices, ball.triangles.astype(int)
    assert len(t) == 80 and len(v) == 42 and ball.normals.shape == (42, 3)
    assert np.allclose(np.linalg.norm(v - np.array([1.0, 2.0, 3.0]), axis=1), 0.5, atol=1e-15)
    assert np.allclose(ball.normals, (v - np.array([1.0, 2.0, 3.0])) / 0.5, atol=1e-15)
    facet = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    assert np.all(np.einsum("ij,ij->i", facet, v[t].mean(axis=1) - np.array([1.0, 2.0, 3.0])) > 0)   # wound outwards
    # 64 quads: consecutive triangles that share their first vertex and an edge (what the leaf records fuse); 16 pole triangles
    quads = sum(1 for k in range(8, 72, 2) if t[k][0] == t[k + 1][0] and t[k][2] == t[k + 1][1])
    assert quads == 32
    assert uv_sphere_mesh(8, 6, smooth=False).normals is None
    # area-weighted normals: a flat grid's are the plane's; a vertex's is the normalised sum of its triangles' e1 x e2
    flat_v = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 1], [0, 0, 1], [5, 5, 5]], dtype=np.float64)
    flat_t = np.array([[0, 2, 1], [0, 3, 2]])
    vn = vertex_normals(flat_v, flat_t)
    assert np.array_equal(vn[:4], np.tile([0.0, 1.0, 0.0], (4, 1))) and np.array_equal(vn[4], [0.0, 1.0, 0.0])   # (unused vertex: the default)
    vn = vertex_normals(v, t)
    want = np.zeros(3)
    for tri in t[(t == 5).any(axis=1)]:
        want = want + np.cross(v[tri[1]] - v[tri[0]], v[tri[2]] - v[tri[0]])
    assert np.allclose(vn[5], want / np.linalg.norm(want), atol=1e-15)
    assert np.allclose(np.linalg.norm(vn, axis=1), 1.0, atol=1e-15)
    # the height field: flat by default (configuration 5's scene as it was), smooth on request
    assert heightfield_mesh(6, 4).normals is None
    hf = heightfield_mesh(6, 4, smooth=True)
    assert hf.normals.shape == (35, 3) and np.array_equal(hf.vertices, heightfield_mesh(6, 4).vertices)
    assert np.all(hf.normals[:, 1] > 0.5)


def test_demo_scene_loads(flux):
    from flux_amd.scene import MeshData, corner_normals
    sd = flux.load_scene(os.path.join(SCENES, "smooth_sphere.yml"))
    meshes = [s for s in sd.shapes if isinstance(s, MeshData)]
    assert len(meshes) == 4
    assert [m.normals is not None for m in meshes] == [True, False, True, False]
    for a, b in ((meshes[0], meshes[1]), (meshes[2], meshes[3])):   # a smooth sphere beside its facetted twin
        assert np.array_equal(a.triangles, b.triangles) and a.material == b.material
        assert corner_normals(a).shape == (len(a.triangles), 3, 3)


# ---- the entry point without a device, the host half stand-alone ------------------------------------------------------------------

def test_null_context_is_refused_without_a_device(flux):
    checks.null_context_refused(flux, "normals")


def _check_selftest_output(out):
    assert "all ok" in out and "FAILED" not in out
    rows = {line.split()[0]: np.array([float(x) for x in line.split()[1:]]) for line in out.splitlines() if line.startswith(("in ", "out "))}
    corners = rows["in"].reshape(-1, 3, 3)
    assert smooth_spec.check_normals(corners) is None
    assert np.array_equal(rows["out"].reshape(-1, 3, 3), smooth_spec.normalize(corners))   # bit for bit: n / sqrt(n.n), IEEE


def test_host_half_equals_the_spec(tmp_path):
    checks.host_selftest(tmp_path, "smooth_host_selftest", _check_selftest_output, sanitized=False)


def test_host_half_under_asan_and_ubsan(tmp_path):
    checks.host_selftest(tmp_path, "smooth_host_selftest", _check_selftest_output, sanitized=True)
