"""Vertex colours without a GPU: the numpy statement of the rule (tests/color_spec.py) against its own properties,
the loader and the procedural meshes, the entry point's checks that need no device, and the host half of the call
(flux_amd/csrc/flux_mesh_attr.h) as a stand-alone program, plain and under the sanitizers."""
import dataclasses
import os

import numpy as np
import pytest

import color_spec
import mesh_attr_checks as checks
from conftest import SCENES

FLT_MAX = color_spec.FLT_MAX


def _random_hits(rng, m):
    """triangles, stored corner colours (a fifth of the components exactly 0) and rays aimed into the triangles"""
    v0 = rng.uniform(-3, 3, (m, 3))
    e1, e2 = rng.uniform(-2, 2, (m, 3)), rng.uniform(-2, 2, (m, 3))
    colors = rng.uniform(0.0, 1.5, (m, 3, 3))
    colors[rng.uniform(size=colors.shape) < 0.2] = 0.0
    bu = rng.uniform(0, 1, m)
    bv = rng.uniform(0, 1, m) * (1.0 - bu)
    target = v0 + bu[:, None] * e1 + bv[:, None] * e2
    o = target + rng.normal(size=(m, 3)) * 3.0
    return v0, e1, e2, color_spec.store(colors), o, target - o


# ---- the spec -----------------------------------------------------------------------------------------------------------------

def test_a_hit_at_a_vertex_returns_that_corners_colour():
    rng = np.random.default_rng(1)
    k = color_spec.store(rng.uniform(0, 2, (50, 3, 3)))
    for j, (u, v) in enumerate(((0.0, 0.0), (1.0, 0.0), (0.0, 1.0))):
        c = color_spec.interpolate(np.full(50, u), np.full(50, v), k[:, 0], k[:, 1], k[:, 2])
        # k0 + 1 (kj - k0) + 0: one subtraction and one addition of f32 values in f64 -- both exact for values within 2^29 of each other
        assert np.array_equal(c, k[:, j].astype(np.float64))


def test_equal_corners_return_that_colour_exactly():
    rng = np.random.default_rng(2)
    k = color_spec.store(rng.uniform(0, 3, (400, 3, 3)))[:, 0]
    u = rng.uniform(-2, 3, 400)   # (any finite barycentrics, inside the triangle or not)
    v = rng.uniform(-2, 3, 400)
    assert np.array_equal(color_spec.interpolate(u, v, k, k, k), k.astype(np.float64))
    assert np.array_equal(color_spec.interpolate(1e300, -1e300, k[0], k[0], k[0]), k[0].astype(np.float64))


def test_all_ones_colours_give_exactly_one():
    rng = np.random.default_rng(3)
    v0, e1, e2, _, o, d = _random_hits(rng, 2000)
    ones = np.ones((2000, 3, 3), dtype=np.float32)
    assert np.array_equal(color_spec.color_factor(v0, e1, e2, ones, o, d), np.ones((2000, 3)))


def test_the_factor_is_never_negative_on_random_hits():
    rng = np.random.default_rng(4)
    v0, e1, e2, k, o, d = _random_hits(rng, 10000)
    assert (k == 0.0).mean() > 0.1
    c = color_spec.color_factor(v0, e1, e2, k, o, d)
    assert c.shape == (10000, 3) and np.isfinite(c).all() and (c >= 0.0).all()
    assert not np.signbit(c).any()   # (fmax(-0.0, 0.0) may be either zero in IEEE; numpy's and the device's maxNum of a residue below 0 is +0)
    # inside the triangle the factor is a convex combination to rounding
    lo, hi = k.min(axis=1).astype(np.float64), k.max(axis=1).astype(np.float64)
    assert np.all(c >= lo - 1e-9) and np.all(c <= hi + 1e-9)
    # a residue below zero is clamped: corners (0, 0, 1) at barycentrics a rounding step outside
    c = color_spec.interpolate(-1e-17, 0.3, np.zeros(3), np.ones(3), np.zeros(3))
    assert np.array_equal(c, np.zeros(3))


def test_a_nan_never_leaves_it():
    tri = (np.zeros(3), np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]))
    k = color_spec.store(np.array([[[0.2, 0.4, 0.6], [1.0, 0.0, 0.5], [0.3, 0.9, 0.1]]]))[0]
    cases = [(np.array([0.2, 0.2, 1.0]), np.array([1.0, 0.0, 0.0])),       # a ray in the triangle's plane: e1.p = 0, inv = inf, 0 inf = NaN
             (np.array([np.nan, 0.2, 1.0]), np.array([0.0, 0.0, -1.0])),   # a NaN origin
             (np.array([0.2, 0.2, 1.0]), np.array([0.0, 0.0, -np.inf])),   # an infinite direction
             (np.array([0.2, 0.2, 1.0]), np.array([0.0, np.nan, -1.0])),   # a NaN direction
             (np.array([1e308, 1e308, 1.0]), np.array([0.0, 0.0, -1.0]))]  # barycentrics that overflow
    for o, d in cases:
        c = color_spec.color_factor(*tri, k, o, d)
        assert not np.isnan(c).any() and (c >= 0.0).all(), (o, d, c)
    assert np.array_equal(color_spec.color_factor(*tri, k, *cases[0]), np.zeros(3))   # NaN -> 0


def test_checks_and_rounding():
    good = np.array([[[0.1, 0.2, 0.3], [-0.0, 1.0, FLT_MAX], [1e-46, 5e-324, 1e38]]])
    assert color_spec.check_colors(good) is None
    assert color_spec.store(good).dtype == np.float32
    assert np.array_equal(color_spec.store(good)[0, 0], np.array([0.1, 0.2, 0.3], dtype=np.float32))
    for value in (np.nan, -1e-300, -np.inf, np.inf, np.nextafter(FLT_MAX, np.inf), 1e300):
        bad = np.tile(good, (3, 1, 1))
        bad[2, 1, 0] = value
        bad[2, 2, 2] = value
        assert color_spec.check_colors(bad) == (2, 1, 0), value


# ---- the loader, the procedural meshes ------------------------------------------------------------------------------------------

_load = checks.load


def test_colours_round_trip_into_the_calls_layout(flux):
    from flux_amd.scene import corner_colors
    per_vertex = [[0, 0, 1], [0.5, 0, 1], [0.5, 0.5, 2], [0, 0.25, 0.1]]
    sd = _load(flux, f"colors: {per_vertex}")
    mesh = sd.shapes[0]
    assert mesh.colors.shape == (4, 3) and mesh.colors.dtype == np.float64 and mesh.normals is None
    c = corner_colors(mesh)
    assert c.shape == (2, 3, 3) and c.flags["C_CONTIGUOUS"] and c.dtype == np.float64
    want = np.array(per_vertex, dtype=np.float64)[np.array([[0, 1, 2], [0, 2, 3]])]
    assert np.array_equal(c, want)   # not rounded here: the library does that
    assert color_spec.check_colors(c) is None
    per_corner = np.arange(18, dtype=np.float64).reshape(2, 3, 3)   # per corner: taken as given
    assert np.array_equal(corner_colors(dataclasses.replace(mesh, colors=per_corner)), per_corner)
    # absent: None; a Triangle stays plain; MeshData's field is the last, with default None
    assert _load(flux, "").shapes[0].colors is None and corner_colors(_load(flux, "").shapes[0]) is None
    tri = flux.scene.shape_from_yaml({"Triangle": {"v0": [0, 0, 0], "v1": [1, 0, 0], "v2": [0, 1, 0], "colors": [[0, 0, 1]] * 3,
                                                   "material": {"Emissive": {"color": [1, 1, 1], "power": 1.0}}}})
    assert tri.colors is None
    fields = dataclasses.fields(flux.scene.MeshData)
    assert fields[-1].name == "colors" and fields[-1].default is None
    # both attributes at once
    both = _load(flux, f"colors: {per_vertex}\n      normals: [[0, 0, -1], [0, 0, -1], [0, 0, -1], [0, 0, -1]]").shapes[0]
    assert both.colors is not None and both.normals is not None


@pytest.mark.parametrize("line,message", [
    ("colors: [[0, 0, 1], [0, 0, 1], [0, 0, 1]]", "expected one [r,g,b] per vertex (4), got 3"),
    ("colors: 7", "expected one [r,g,b] per vertex (4)"),
    ("colors: [[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, x, 1]]", "colors[3]: expected a sequence of 3 numbers"),
    ("colors: [[0, 0, 1], [0, 0, 1], [0, 0], [0, 0, 1]]", "colors[2]: expected a sequence of 3 numbers"),
    ("colors: [[0, 0, 1], [0, -0.5, 0], [0, 0, 1], [0, 0, 1]]", "triangle 0, corner 1, channel 1: component -0.5 must lie in [0, FLT_MAX]"),
    ("colors: [[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, .inf, 1]]", "triangle 1, corner 2, channel 1"),
    ("colors: [[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 1, .nan]]", "triangle 1, corner 2, channel 2"),
    ("colors: [[0, 0, 1], [0, 0, 1], [1.0e+39, 0, 1], [0, 1, 1]]", "triangle 0, corner 2, channel 0"),
])
def test_loader_refusals(flux, line, message):
    checks.loader_refusal(flux, line, message)


def test_meshdata_refusals(flux):
    from flux_amd.scene import corner_colors
    mesh = checks.meshdata_refusals(flux, "colors", np.full((4, 3), -1e-300), "mesh 0.colors: triangle 0, corner 0, channel 0")
    # the loader's verdict is the spec's, offender for offender
    rng = np.random.default_rng(5)
    for _ in range(20):
        c = rng.uniform(0, 1, (2, 3, 3))
        c[tuple(rng.integers(0, s) for s in c.shape)] = rng.choice([np.nan, -1.0, np.inf, 4e38])
        k, j, ch = color_spec.check_colors(c)
        with pytest.raises(flux.SceneError) as e:
            corner_colors(dataclasses.replace(mesh, colors=c))
        assert f"triangle {k}, corner {j}, channel {ch}:" in str(e.value)


def test_procedural_meshes(flux):
    from flux_amd.procedural import elevation_colors, heightfield_mesh, heightfield_scene, uv_sphere_mesh
    v = np.array([[0, -1.0, 0], [1, 1.0, 0], [2, 0.0, 5], [3, 0.5, 1]])
    c = elevation_colors(v, (0.0, 0.2, 1.0), (1.0, 0.2, 0.0))
    assert np.array_equal(c[0], [0.0, 0.2, 1.0]) and np.array_equal(c[1], [1.0, 0.2, 0.0])
    assert np.allclose(c[2], [0.5, 0.2, 0.5]) and np.allclose(c[3], [0.75, 0.2, 0.25])
    assert np.array_equal(elevation_colors(np.zeros((3, 3)), (0.1, 0.2, 0.3), (1, 1, 1)), np.tile([0.1, 0.2, 0.3], (3, 1)))   # one height
    # the defaults keep the meshes as they were
    assert heightfield_mesh(6, 4).colors is None and uv_sphere_mesh(8, 6).colors is None
    hf = heightfield_mesh(6, 4, colored=True)
    assert hf.colors.shape == (35, 3) and hf.normals is None and np.array_equal(hf.vertices, heightfield_mesh(6, 4).vertices)
    assert color_spec.check_colors(hf.colors[hf.triangles.astype(int)]) is None and np.ptp(hf.colors, axis=0).max() > 0.5
    plain, colored = heightfield_scene(6, 4), heightfield_scene(6, 4, colored=True)
    assert plain.shapes[-1].colors is None and colored.shapes[-1].colors is not None
    assert plain.scene_name == colored.scene_name and len(plain.shapes) == len(colored.shapes)
    ball = uv_sphere_mesh(8, 6, colors=np.full((42, 3), 0.5))
    assert ball.colors.shape == (42, 3) and ball.normals is not None


def test_demo_scene_loads(flux):
    from flux_amd.scene import MeshData, corner_colors
    sd = flux.load_scene(os.path.join(SCENES, "vertex_colors.yml"))
    meshes = [s for s in sd.shapes if isinstance(s, MeshData)]
    assert [(m.normals is not None, m.colors is not None) for m in meshes] == [(True, True), (False, True)]
    ball, floor = meshes
    assert corner_colors(ball).shape == (len(ball.triangles), 3, 3) and len(floor.triangles) == 128
    fc = corner_colors(floor)
    assert (fc == fc[:, :1]).all()                  # a checker: every cell one colour ...
    assert len({tuple(x) for x in fc[:, 0]}) == 2   # ... of two


def test_render_frame_multi_refuses_a_coloured_mesh(flux):
    sd = _load(flux, "colors: [[0, 0, 1], [0.5, 0, 1], [0.5, 0.5, 1], [0, 0.25, 0.1]]")
    with pytest.raises(flux.FluxError) as e:
        flux.render_frame_multi(sd, flux.JobConfiguration(2, 2, 50))
    assert "vertex colours" in str(e.value)


# ---- the entry point without a device, the host half stand-alone ------------------------------------------------------------------

def test_null_context_is_refused_without_a_device(flux):
    checks.null_context_refused(flux, "colors")


def _check_selftest_output(out):
    assert "all ok" in out and "FAILED" not in out
    rows = {line.split()[0]: [float(x) for x in line.split()[1:]] for line in out.splitlines() if line.startswith(("in ", "out "))}
    corners = np.array(rows["in"]).reshape(-1, 3, 3)
    assert color_spec.check_colors(corners) is None
    got = np.array(rows["out"]).astype(np.float32).reshape(-1, 3, 3)   # (%.9g round-trips an f32)
    assert got.tobytes() == color_spec.store(corners).tobytes()        # bit for bit: numpy's astype(float32), -0.0 included


def test_host_half_equals_the_spec(tmp_path):
    checks.host_selftest(tmp_path, "color_host_selftest", _check_selftest_output, sanitized=False)


def test_host_half_under_asan_and_ubsan(tmp_path):
    checks.host_selftest(tmp_path, "color_host_selftest", _check_selftest_output, sanitized=True)
