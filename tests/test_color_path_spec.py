"""tests/color_path_spec.py, the full-path reference of the vertex-colour GPU tests, held against tests/smooth_path_spec.py before
it judges a kernel: without colours it IS SmoothPathSpec, with all-ones colours on every mesh it is again, bit for bit, and no scene
or debug ray the GPU tests use takes a decision at rounding level.  No GPU."""
import copy

import numpy as np
import pytest

import color_path_spec
import color_scenes
import path_spec
import smooth_path_spec
import smooth_scenes

MARGIN = 1e-9


def _same(spec, ref):
    assert np.array_equal(spec.frame(), ref.frame(), equal_nan=True)
    assert spec.stats == ref.stats and spec.classes == ref.classes
    assert spec.margins == ref.margins


def _all_ones(sd):
    out = copy.deepcopy(sd)
    for s in out.shapes:
        if type(s).__name__ == "MeshData":
            s.colors = np.ones((len(s.triangles), 3, 3))
    return out


@pytest.mark.parametrize("material,root", smooth_scenes.GPU_JOBS)
def test_without_colours_and_with_all_ones_it_is_the_smooth_reference(material, root):
    """Every job of tests/smooth_scenes.py: the restated loop is SmoothPathSpec's (frame, statistics, classes, margins), and a factor
    of exactly 1 on every triangle hit changes no bit."""
    sd, seed, ref = smooth_scenes.reference(material, root)
    for variant in (sd, _all_ones(sd)):
        spec = color_path_spec.ColorPathSpec(variant, root, smooth_scenes.DEPTH, seed)
        try:
            _same(spec, ref)
            assert np.array_equal(color_path_spec.aov_buffers(spec), path_spec.aov_buffers(ref))
            factors = [f for f in spec.first_factors() if f is not None]
            if variant is sd:
                assert not factors
            else:
                assert factors and all(np.array_equal(f, np.ones(3)) for f in factors)
        finally:
            spec.close()


def test_the_chain_twin_is_the_chain_reference_without_colours():
    import aov_chain_spec
    sd, seed, ref = smooth_scenes.reference("Dielectric", 2)
    for variant in (sd, _all_ones(sd)):
        spec = color_path_spec.ColorPathSpec(variant, 2, smooth_scenes.DEPTH, seed)
        try:
            got, margins = color_path_spec.chain_buffers(spec, 0)
            want = aov_chain_spec.chain_buffers(ref, 0)
            assert np.array_equal(got, want.buffers, equal_nan=True) and margins == want.margins
        finally:
            spec.close()


def test_every_coloured_triangle_has_corners_that_differ():
    import flux_amd as flux
    sd = color_scenes.scene(flux, "Matte")
    assert color_scenes.spread(sd.shapes[3]) >= 0.3 and color_scenes.spread(sd.shapes[4]) >= 0.3
    assert sd.shapes[3].normals is not None and sd.shapes[4].normals is None
    assert sd.shapes[5].normals is None and sd.shapes[5].colors is None
    assert (color_scenes.sphere_colors() == 0.0).any()
    assert color_scenes.spread(color_scenes.c_client_scene(flux).shapes[2]) >= 0.3


@pytest.mark.parametrize("material,root", color_scenes.GPU_JOBS)
def test_no_gpu_scene_decides_at_rounding_level(material, root):
    """What lets tests/test_gpu_vertex_colors.py demand equal statistics and exclude nothing: the condition the smooth suite imposes"""
    sd, seed, spec = color_scenes.reference(material, root)
    assert set(spec.margins) == set(path_spec.MARGIN_NAMES) | set(smooth_path_spec.MARGIN_NAMES_SMOOTH)
    low = {k: v for k, v in spec.margins.items() if not v > MARGIN}
    assert not low, (material, root, seed, low)
    assert spec.classes[f"Mesh/{type(sd.shapes[3].material).__name__[:-4]}"] > 0, spec.classes
    factors = [f for f in spec.first_factors() if f is not None]
    assert factors and np.min(factors) >= 0.0 and np.ptp(np.array(factors), axis=0).max() > 0.3   # the scene does interpolate colours
    # ... and the colours matter: the frame is not the plain scene's
    plain = smooth_path_spec.SmoothPathSpec(color_scenes.plain_twin(sd), root, color_scenes.DEPTH, seed) if root == 2 else None
    if plain is not None:
        try:
            assert not np.array_equal(plain.frame(), spec.frame())
            assert plain.stats == spec.stats   # (a colour changes no decision of a path)
        finally:
            plain.close()


@pytest.mark.parametrize("material", color_scenes.MESH_MATERIALS)
def test_no_debug_ray_decides_at_rounding_level(material):
    o, d, _, _, rad, t, margins = color_scenes.debug_reference(material)
    low = {k: v for k, v in margins.items() if not v > MARGIN}
    assert not low, (material, low)
    assert np.isfinite(rad).all() and np.isfinite(t).mean() > 0.9   # the rays are aimed at the meshes


def test_the_scene_shades_every_kind_of_triangle():
    """Depth-1 hits on the sphere's quads and pole triangles (normals and colours), on both floor triangles (colours only) and on
    the wall (neither); pixels of the wall alone and of the floor's checker."""
    sd, seed, spec = color_scenes.reference("Matte", 8)
    o, d, _ = spec.primary
    shape, _, _ = spec.first_hits()
    hit = set()
    for r, c, i in zip(*np.nonzero(shape >= 3)):
        hit.add(spec.triangle_of(o[r, c, i], d[r, c, i]))
    ball = {k for k in hit if k < 80}
    assert any(k < 8 or k >= 72 for k in ball) and any(8 <= k < 72 and k % 2 == 0 for k in ball) and any(8 <= k < 72 and k % 2 for k in ball)
    assert {80, 81} <= hit and hit & {82, 83}, sorted(hit)
    assert (shape == 5).all(axis=2).sum() >= 2 and (shape == 3).all(axis=2).any() and (shape == 4).all(axis=2).any()
