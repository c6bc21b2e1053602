"""Vertex colours on the GPU: every kernel that shades a triangle, in both arithmetics and over the three
traversals, against tests/color_path_spec.py -- the feature buffers, the paths, flux_debug_shade, all-ones colours and set / clear
against contexts that never had them, the meshes without colours left alone, every consumer, the shares, the C ABI from plain C,
the refusals.  The scenes are tests/color_scenes.py's: tests/smooth_scenes.py's 12 x 9 scene whose 80-triangle sphere has normals and
colours, whose floor has a per-corner checker and no normals, whose wall has neither; sample roots 2, 8 and 16.
tests/test_color_path_spec.py shows that no decision of these scenes lies within 1e-9 of its threshold, so nothing is excluded."""
import itertools

import numpy as np
import pytest

import aov_spec
import color_path_spec
import color_scenes
import mesh_attr_checks as checks
import test_gpu_ext_fuzz as fuzz
from mesh_attr_checks import (assert_same as _assert_same, configurations as _configurations, configure as _configure,
                              everything as _everything, traversals as _traversals)

pytestmark = pytest.mark.gpu

ALBEDO_TOL = 1e-12   # the issue's: a few ulp per sample over at most 256 samples of values <= 1; a wrong corner moves a pixel mean by >= 1e-3
NORMAL_TOL = 1e-12   # the smooth suite's
TRIANGLES = 84       # 80 + 2 + 2: the table holds a record for every triangle of the scene
TIGHT = ((aov_spec.ALBEDO, ALBEDO_TOL), (aov_spec.NORMAL, NORMAL_TOL))


def _renderer(flux, sd, root, seed):
    return checks.renderer(flux, sd, root, seed, color_scenes.DEPTH)


# ---- 1. the feature buffers -----------------------------------------------------------------------------------------------------

def _assert_aov(got, want, label):
    checks.assert_aov(got, want, f"colour aov {label}", TIGHT)


@pytest.mark.parametrize("material,root", [("Matte", 2), ("Matte", 8), ("Matte", 16), ("Dielectric", 2), ("Reflective", 2), ("Emissive", 2)])
def test_feature_buffers(flux, material, root):
    sd, seed, spec = color_scenes.reference(material, root)
    first = color_path_spec.aov_buffers(spec)
    chain, margins = color_path_spec.chain_buffers(spec, 0)
    assert min(margins.values()) > 1e-9   # (the chain's own decisions past the first hit)
    with _renderer(flux, sd, root, seed) as r:
        for math, trav in itertools.product((flux.MATH_FAST, flux.MATH_STRICT), _traversals(flux)):
            r.set_math(math)
            r.set_traversal(trav)
            _assert_aov(r.render_aov(), first, f"{material} root {root} math {math} traversal {trav} first hit")
            _assert_aov(r.render_aov_chain(), chain, f"{material} root {root} math {math} traversal {trav} chain")
    if material in ("Dielectric", "Reflective"):
        assert not np.array_equal(first, chain)   # the chain does go through the coloured sphere


# ---- 2. the paths, 3. flux_debug_shade --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("material,root", color_scenes.GPU_JOBS)
def test_frames_against_the_path_reference(flux, material, root):
    """Every kernel that takes a mesh: all ten statistics equal, the frame within test_gpu_ext_fuzz's tolerances (check_run)"""
    sd, seed, spec = color_scenes.reference(material, root)
    worst = {}
    with _renderer(flux, sd, root, seed) as r:
        for math, kernel, trav in _configurations(flux):
            _configure(r, math, kernel, trav)
            fuzz.check_run(flux, r, spec, f"{material} root {root} math {math} kernel {kernel} traversal {trav}", True, worst)
    print(f"colour {material} root {root}: max |gpu - reference| " + ", ".join(f"{k} {v:.3e}" for k, v in sorted(worst.items())))


@pytest.mark.parametrize("material", color_scenes.MESH_MATERIALS)
def test_debug_shade_against_the_path_reference(flux, material):
    checks.debug_shade(flux, color_scenes, "colour", material)


# ---- 4. all-ones colours ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("material,root", tuple((m, 2) for m in color_scenes.MESH_MATERIALS) + (("Matte", 8), ("Matte", 16)))
def test_all_ones_colours_change_no_bit(flux, material, root):
    """c = 1 exactly, in both arithmetics: frame, statistics, feature buffers, chain buffers and moments of a context with all-ones
    colours on every mesh equal those of a context that never had colours, in every configuration"""
    seed = color_scenes.job_seed(material, root)
    ones, never = color_scenes.scene(flux, material, "ones"), color_scenes.scene(flux, material, None)
    with _renderer(flux, ones, root, seed) as a, _renderer(flux, never, root, seed) as b:
        assert a.device_bytes() == b.device_bytes()   # (the sphere's normals hold the table in both)
        for cfg in _configurations(flux):
            _configure(a, *cfg)
            _configure(b, *cfg)
            _assert_same(_everything(a), _everything(b), (material, root, cfg))
    # ... and without any normals: the table exists for the colours alone
    ones, never = color_scenes.scene(flux, material, "ones", normals=False), color_scenes.scene(flux, material, None, normals=False)
    with _renderer(flux, ones, root, seed) as a, _renderer(flux, never, root, seed) as b:
        assert a.device_bytes() == b.device_bytes() + TRIANGLES * 128
        for cfg in _configurations(flux):
            _configure(a, *cfg)
            _configure(b, *cfg)
            _assert_same(_everything(a), _everything(b), (material, root, cfg, "no normals"))


# ---- 5. set and clear in every order ------------------------------------------------------------------------------------------------

ORDERS = (("C+", "N+", "N-", "C-"), ("N+", "C+", "C-", "N-"), ("C+", "N+", "C-", "N-"), ("N+", "C+", "N-", "C-"))


@pytest.mark.parametrize("root", [2, 8])
def test_set_and_clear_in_every_order(flux, root):
    """After each step the context equals a fresh one that had only what is set at that point; the table costs 128 B per triangle for
    the first attribute and nothing for the second; the launch plan never moves"""
    seed = color_scenes.job_seed("Glossy", 2)
    full = color_scenes.scene(flux, "Glossy")
    ball, floor = full.shapes[3], full.shapes[4]
    fresh = {}
    for normals, colors in itertools.product((False, True), (False, True)):
        with _renderer(flux, color_scenes.scene(flux, "Glossy", "on" if colors else None, normals), root, seed) as r:
            fresh[(normals, colors)] = (_everything(r), r.device_bytes(), r.launch_plan(flags=True))
    bytes0 = fresh[(False, False)][1]
    assert len({np.asarray(v[0][0]).tobytes() for v in fresh.values()}) == 4   # four different frames
    assert all(v[2] == fresh[(False, False)][2] for v in fresh.values())
    for order in ORDERS:
        with _renderer(flux, color_scenes.scene(flux, "Glossy", None, False), root, seed) as r:
            state = [False, False]
            for step in order:
                if step[0] == "N":
                    r.set_mesh_normals(0, ball.normals if step[1] == "+" else None)
                    state[0] = step[1] == "+"
                else:
                    r.set_mesh_colors(0, ball.colors if step[1] == "+" else None)
                    r.set_mesh_colors(1, floor.colors if step[1] == "+" else None)   # (per corner)
                    r.set_mesh_colors(2, None)                                       # (clearing a mesh that has none: nothing to do)
                    state[1] = step[1] == "+"
                want, size, plan = fresh[tuple(state)]
                assert r.device_bytes() == size == bytes0 + (TRIANGLES * 128 if any(state) else 0), (order, step)
                assert r.launch_plan(flags=True) == plan
                _assert_same(_everything(r), want, (order, step))
            assert r.device_bytes() == bytes0
    # replacing: the second call's colours stand
    with _renderer(flux, full, root, seed) as r:
        r.set_mesh_colors(0, np.ones((80, 3, 3)))
        r.set_mesh_colors(0, ball.colors)
        _assert_same(_everything(r), fresh[(True, True)][0], "replaced")


# ---- 6. isolation -------------------------------------------------------------------------------------------------------------------

def test_wall_pixels_do_not_see_the_other_meshes_colours(flux):
    sd, seed, spec = color_scenes.reference("Matte", 8)
    shape, _, _ = spec.first_hits()
    only_wall = (shape == 5).all(axis=2)
    assert only_wall.sum() >= 2, only_wall.sum()
    with _renderer(flux, sd, 8, seed) as r, _renderer(flux, color_scenes.plain_twin(sd), 8, seed) as f:
        for math, trav in itertools.product((flux.MATH_FAST, flux.MATH_STRICT), _traversals(flux)):
            for x in (r, f):
                x.set_math(math)
                x.set_traversal(trav)
            a, b = r.render_aov(), f.render_aov()
            assert np.array_equal(a[only_wall], b[only_wall])
            assert not np.array_equal(a[~only_wall], b[~only_wall])


# ---- 7. every consumer ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("root", [2, 8])
def test_every_consumer_sees_the_colours(flux, root):
    checks.every_consumer(flux, color_scenes, color_scenes.plain_twin, root, aov_spec.ALBEDO, 4, 0.2,
                          "coloured against plain albedo buffer on the checker floor")


# ---- 8. shares ------------------------------------------------------------------------------------------------------------------

def test_shares_give_the_renderers_frame(flux):
    checks.shares(flux, color_scenes, color_scenes.plain_twin)   # (the one call refuses a coloured mesh)


# ---- 9. the C ABI from plain C --------------------------------------------------------------------------------------------------

def test_c_client_sets_colours_and_is_refused_as_the_header_says(flux, tmp_path):
    checks.c_client(flux, tmp_path, "color_c_client", color_scenes, color_scenes.plain_twin, "plain", "colored")


# ---- 10. refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals_on_a_live_context_leave_it_unchanged(flux):
    sd, seed, _ = color_scenes.reference("Matte", 2)
    with _renderer(flux, sd, 2, seed) as r:
        frame, aov, size = r.render_frame(), r.render_aov(), r.device_bytes()
        good = np.tile(np.array([0.5, 1.0, 0.25]), (80, 3, 1))
        refusal = checks.common_refusals(flux, r, "colors", good)
        for value, where in ((-1e-9, (17, 2, 1)), (np.nan, (0, 0, 0)), (np.inf, (79, 1, 2)), (-np.inf, (40, 0, 1)), (3.5e38, (3, 2, 0))):
            bad = good.copy()
            bad[where] = value
            message = refusal(0, bad, 80)
            assert f"mesh 0, triangle {where[0]}, corner {where[1]}, channel {where[2]}" in message, message
        with pytest.raises(flux.SceneError):
            r.set_mesh_colors(0, np.zeros((42, 2)))
        with pytest.raises(flux.SceneError):
            r.set_mesh_colors(0, np.full((42, 3), -1.0))
        with pytest.raises(flux.FluxError):
            r.set_mesh_colors(7, None)
        assert r.device_bytes() == size
        assert np.array_equal(r.render_frame(), frame) and np.array_equal(r.render_aov(), aov)
    # a context of flux_ctx_create_sets takes the call as well
    with flux.Renderer(sd, flux.JobConfiguration(2, color_scenes.DEPTH, 50), seed=seed, set_share=(1, 2)) as share:
        share.set_mesh_colors(0, None)
        share.set_mesh_colors(0, sd.shapes[3].colors)
