"""tests/smooth_path_spec.py, the full-path reference of the smooth-mesh GPU tests, held against tests/path_spec.py before it judges
a kernel: without normals it IS PathSpec, with every corner set to its facet normal it agrees with it to rounding, and no scene
the GPU tests use takes a decision at rounding level.  No GPU."""
import copy

import numpy as np
import pytest

import path_spec
import smooth_path_spec
import smooth_scenes
import smooth_spec
import test_gpu_ext_fuzz as fuzz

MARGIN = 1e-9


@pytest.mark.parametrize("chunk", range(fuzz.MESH_CHUNKS))
def test_without_normals_it_is_the_path_reference(chunk):
    for sd, n, D, seed, ref in fuzz.chunk_references(chunk, True):
        spec = smooth_path_spec.SmoothPathSpec(sd, n, D, seed)
        try:
            assert np.array_equal(spec.frame(), ref.frame(), equal_nan=True)
            assert spec.stats == ref.stats and spec.classes == ref.classes
            assert {k: v for k, v in spec.margins.items() if k != "smooth_l2"} == ref.margins
            assert spec.margins["smooth_l2"] == np.inf   # nothing was interpolated
        finally:
            spec.close()


def _with_facet_normals(sd):
    """`sd` with every mesh given its own facet normals as corner normals ((0, 1, 0) for a triangle without area, which is never hit)"""
    out = copy.deepcopy(sd)
    for s in out.shapes:
        if type(s).__name__ == "MeshData":
            facet = smooth_spec.mesh_triangles(s)[3]
            facet = np.where((facet == 0.0).all(axis=1)[:, None], np.array([0.0, 1.0, 0.0]), facet)
            s.normals = np.repeat(facet[:, None, :], 3, axis=1)
    return out


@pytest.mark.parametrize("chunk", range(fuzz.MESH_CHUNKS))
def test_facet_normals_as_corner_normals_change_nothing(chunk):
    """m = (w n + u n) + v n is n to rounding and m / |m| a unit vector to rounding: per bounce a relative 1e-15 or so, far below
    1e-12 through a path of at most nine."""
    for sd, n, D, seed, ref in fuzz.chunk_references(chunk, True):
        spec = smooth_path_spec.SmoothPathSpec(_with_facet_normals(sd), n, D, seed)
        try:
            got, want = spec.frame(), ref.frame()
            assert spec.stats == ref.stats
            finite = np.isfinite(want)
            assert np.array_equal(np.isfinite(got), finite)
            scale = np.maximum(1.0, np.abs(want[finite]))
            assert not finite.any() or np.max(np.abs(got[finite] - want[finite]) / scale) <= 1e-12
            if ref.classes and any(k.startswith("Mesh/") for k in ref.classes):
                assert abs(spec.margins["smooth_l2"] - 1.0) < 1e-12   # every interpolated normal had length 1
        finally:
            spec.close()


@pytest.mark.parametrize("material,root", smooth_scenes.GPU_JOBS)
def test_no_gpu_scene_decides_at_rounding_level(material, root):
    """What lets tests/test_gpu_smooth_normals.py demand equal statistics and exclude nothing: PathSpec's margins and l2 against 1e-24."""
    sd, seed, spec = smooth_scenes.reference(material, root)
    assert set(spec.margins) == set(path_spec.MARGIN_NAMES) | set(smooth_path_spec.MARGIN_NAMES_SMOOTH)
    low = {k: v for k, v in spec.margins.items() if not v > MARGIN}
    assert not low, (material, root, seed, low)
    assert spec.margins["smooth_l2"] < np.inf   # the scene does interpolate
    assert spec.classes[f"Mesh/{type(sd.shapes[3].material).__name__[:-4]}"] > 0, spec.classes   # ... and on the sphere's material


@pytest.mark.parametrize("material", smooth_scenes.MESH_MATERIALS)
def test_no_debug_ray_decides_at_rounding_level(material):
    o, d, _, _, rad, t, margins = smooth_scenes.debug_reference(material)
    low = {k: v for k, v in margins.items() if not v > MARGIN}
    assert not low, (material, low)
    assert np.isfinite(rad).all() and np.isfinite(t).mean() > 0.9   # the rays are aimed at the meshes


def test_the_scene_shades_both_record_kinds_and_the_flat_mesh():
    """The 80-triangle sphere's quads and pole triangles, the floor and the mesh without normals are all hit at depth 1."""
    sd, seed, spec = smooth_scenes.reference("Matte", 8)
    o, d, _ = spec.primary
    shape, _, _ = spec.first_hits()
    hit = set()
    for r, c, i in zip(*np.nonzero(shape >= 3)):
        hit.add(spec.triangle_of(o[r, c, i], d[r, c, i]))
    ball = {k for k in hit if k < 80}
    assert any(k < 8 or k >= 72 for k in ball) and any(8 <= k < 72 and k % 2 == 0 for k in ball) and any(8 <= k < 72 and k % 2 for k in ball)
    assert hit & {80, 81} and hit & {82, 83}, sorted(hit)
    assert (shape == 5).all(axis=2).sum() >= 2 and (shape == 3).all(axis=2).any()   # pixels of the flat mesh alone, and of the sphere alone
    assert (smooth_scenes.reference("Matte", 2)[2].first_hits()[0] == 3).all(axis=2).any()
