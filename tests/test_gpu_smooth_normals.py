"""Smooth meshes on the GPU: every kernel that takes a mesh, in both arithmetics and over the three traversals,
against tests/smooth_path_spec.py -- the feature buffers, the paths, the flat path left as it was, every consumer of the normal, the
shares, the C ABI from plain C and the launch plan.  The scenes are tests/smooth_scenes.py's: 12 x 9 pixels, an 80-triangle UV sphere
with normals (quads that fuse into two-triangle leaf records, pole triangles that do not), a floor quad with tilted normals, a mesh
WITHOUT normals, an analytic sphere and plane, an inverted Emissive environment; sample roots 2, 8 and 16.
tests/test_smooth_path_spec.py shows that no decision of these scenes lies within 1e-9 of its threshold, so nothing is excluded."""
import itertools

import numpy as np
import pytest

import aov_chain_spec
import aov_spec
import mesh_attr_checks as checks
import path_spec
import smooth_scenes
import test_gpu_ext_fuzz as fuzz
from mesh_attr_checks import configurations as _configurations, everything as _everything, traversals as _traversals

pytestmark = pytest.mark.gpu

NORMAL_TOL = 1e-12   # the issue's: a few ulp per sample over at most 256 samples; a swapped or dropped corner moves a sample by > 0.1
TIGHT = ((aov_spec.NORMAL, NORMAL_TOL),)


def _renderer(flux, sd, root, seed):
    return checks.renderer(flux, sd, root, seed, smooth_scenes.DEPTH)


# ---- 1. the feature buffers -----------------------------------------------------------------------------------------------------

def _assert_aov(got, want, label):
    checks.assert_aov(got, want, f"smooth aov {label}", TIGHT)


@pytest.mark.parametrize("material,root", [("Matte", 2), ("Matte", 8), ("Matte", 16), ("Dielectric", 2), ("Emissive", 2)])
def test_feature_buffers(flux, material, root):
    sd, seed, spec = smooth_scenes.reference(material, root)
    first = path_spec.aov_buffers(spec)
    chain = aov_chain_spec.chain_buffers(spec, 0)
    assert min(chain.margins.values()) > 1e-9   # (the chain's own decisions: the glass scene's Fresnel draws past the first hit)
    with _renderer(flux, sd, root, seed) as r:
        for math, trav in itertools.product((flux.MATH_FAST, flux.MATH_STRICT), _traversals(flux)):
            r.set_math(math)
            r.set_traversal(trav)
            _assert_aov(r.render_aov(), first, f"{material} root {root} math {math} traversal {trav} first hit")
            _assert_aov(r.render_aov_chain(), chain.buffers, f"{material} root {root} math {math} traversal {trav} chain")
    if material == "Dielectric":
        assert not np.array_equal(first, chain.buffers)   # the chain does go through the glass sphere


# ---- 2. the paths ---------------------------------------------------------------------------------------------------------------

def _frames(flux, r):
    out = {}
    for math, kernel, trav in _configurations(flux):
        checks.configure(r, math, kernel, trav)
        out[(math, kernel, trav)] = r.render_frame()
    return out


@pytest.mark.parametrize("material,root", smooth_scenes.GPU_JOBS)
def test_frames_against_the_path_reference(flux, material, root):
    """Every kernel that takes a mesh: all ten statistics equal, the frame within test_gpu_ext_fuzz's tolerances (check_run); and two
    configurations give bit-equal frames wherever they do on the same scene without normals."""
    sd, seed, spec = smooth_scenes.reference(material, root)
    worst, smooth = {}, {}
    with _renderer(flux, sd, root, seed) as r:
        for math, kernel, trav in _configurations(flux):
            checks.configure(r, math, kernel, trav)
            smooth[(math, kernel, trav)], _ = fuzz.check_run(flux, r, spec, f"{material} root {root} math {math} kernel {kernel} traversal {trav}",
                                                             True, worst)
    print(f"smooth {material} root {root}: max |gpu - reference| " + ", ".join(f"{k} {v:.3e}" for k, v in sorted(worst.items())))
    with _renderer(flux, smooth_scenes.flat_twin(sd), root, seed) as r:
        flat = _frames(flux, r)
    pairs = 0
    for a, b in itertools.combinations(_configurations(flux), 2):
        if np.array_equal(flat[a], flat[b], equal_nan=True):
            pairs += 1
            assert np.array_equal(smooth[a], smooth[b], equal_nan=True), (a, b)
    assert pairs > 0
    assert not np.array_equal(smooth[_configurations(flux)[0]], flat[_configurations(flux)[0]])


@pytest.mark.parametrize("material", smooth_scenes.MESH_MATERIALS)
def test_debug_shade_against_the_path_reference(flux, material):
    """2 000 rays per material (10^4 in all) aimed at points of the three meshes: radiance within check_run's tolerances, t equal to
    rounding."""
    checks.debug_shade(flux, smooth_scenes, "smooth", material)


# ---- 3. the flat path is untouched ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("root", [2, 8])
def test_set_and_cleared_equals_never_set(flux, root):
    from flux_amd.scene import corner_normals
    sd, seed, _ = smooth_scenes.reference("Glossy", 2)
    flat_sd = smooth_scenes.flat_twin(sd)
    with _renderer(flux, flat_sd, root, seed) as never, _renderer(flux, flat_sd, root, seed) as r:
        want = _everything(never)
        bytes0 = r.device_bytes()
        assert bytes0 == never.device_bytes()
        r.set_mesh_normals(0, sd.shapes[3].normals)
        r.set_mesh_normals(1, corner_normals(sd.shapes[4]))   # (per corner)
        assert r.device_bytes() == bytes0 + 84 * 128
        during = _everything(r)
        assert not np.array_equal(during[0], want[0]) and not np.array_equal(during[2], want[2])
        r.set_mesh_normals(0, None)
        assert r.device_bytes() == bytes0 + 84 * 128   # the floor still has its normals
        r.set_mesh_normals(1, None)
        r.set_mesh_normals(2, None)                    # (clearing a mesh that has none: nothing to do)
        assert r.device_bytes() == bytes0
        got = _everything(r)
        for a, b in zip(got, want):
            assert a == b if isinstance(a, dict) else np.array_equal(a, b, equal_nan=True)
    # set after creation == set at creation
    with _renderer(flux, sd, root, seed) as at_creation:
        assert np.array_equal(at_creation.render_frame(), during[0]) and np.array_equal(at_creation.render_aov(), during[2])


def test_flat_mesh_pixels_do_not_see_the_other_meshes_normals(flux):
    """A scene that is the flat mesh alone in front of a black background and a Matte-free set of emitters: pixels whose every sample's
    path touches only it.  Here: the first-hit buffers, which depend on the first hit alone -- every pixel fully covered by the flat
    mesh is bit-equal with and without the other meshes' normals, in both arithmetics and every traversal."""
    sd, seed, spec = smooth_scenes.reference("Matte", 8)
    shape, _, _ = spec.first_hits()
    only_wall = (shape == 5).all(axis=2)
    assert only_wall.sum() >= 2, only_wall.sum()
    with _renderer(flux, sd, 8, seed) as r, _renderer(flux, smooth_scenes.flat_twin(sd), 8, seed) as f:
        for math, trav in itertools.product((flux.MATH_FAST, flux.MATH_STRICT), _traversals(flux)):
            for x in (r, f):
                x.set_math(math)
                x.set_traversal(trav)
            a, b = r.render_aov(), f.render_aov()
            assert np.array_equal(a[only_wall], b[only_wall])
            assert not np.array_equal(a[~only_wall], b[~only_wall])
    # ... and whole paths: the wall alone among emitters (no other mesh to bounce off), beside a smooth sphere nobody can reach
    lone = smooth_scenes.lone_wall_scene(flux)
    with _renderer(flux, lone, 8, seed) as r, _renderer(flux, smooth_scenes.flat_twin(lone), 8, seed) as f:
        for kernel in (flux.KERNEL_DEFAULT, flux.KERNEL_STATIC, flux.KERNEL_REFILL):
            r.set_kernel(kernel)
            f.set_kernel(kernel)
            assert np.array_equal(r.render_frame(), f.render_frame())
        assert r.launch_plan() == f.launch_plan()


# ---- 4. every consumer sees the new normal ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("root", [2, 8])
def test_every_consumer_sees_the_new_normal(flux, root):
    checks.every_consumer(flux, smooth_scenes, smooth_scenes.flat_twin, root, aov_spec.NORMAL, 3, 0.05,
                          "smooth against flat normal buffer on the sphere")


# ---- 5. shares ------------------------------------------------------------------------------------------------------------------

def test_shares_give_the_renderers_frame(flux):
    checks.shares(flux, smooth_scenes, smooth_scenes.flat_twin)


# ---- 6. the C ABI from plain C --------------------------------------------------------------------------------------------------

def test_c_client_sets_normals_and_is_refused_as_the_header_says(flux, tmp_path):
    checks.c_client(flux, tmp_path, "smooth_c_client", smooth_scenes, smooth_scenes.flat_twin, "flat", "smooth")


def test_refusals_on_a_live_context_leave_it_unchanged(flux):
    sd, seed, _ = smooth_scenes.reference("Matte", 2)
    with _renderer(flux, sd, 2, seed) as r:
        frame, aov, size = r.render_frame(), r.render_aov(), r.device_bytes()
        good = np.tile(np.array([0.0, 1.0, 0.0]), (80, 3, 1))
        refusal = checks.common_refusals(flux, r, "normals", good)
        for value, where in ((0.0, (17, 2)), (np.nan, (0, 0)), (np.inf, (79, 1))):
            bad = good.copy()
            bad[where] = value
            message = refusal(0, bad, 80)
            assert f"mesh 0, triangle {where[0]}, corner {where[1]}" in message, message
        with pytest.raises(flux.SceneError):
            r.set_mesh_normals(0, np.zeros((42, 3)))
        with pytest.raises(flux.FluxError):
            r.set_mesh_normals(7, None)
        assert r.device_bytes() == size
        assert np.array_equal(r.render_frame(), frame) and np.array_equal(r.render_aov(), aov)
    # a context of flux_ctx_create_sets takes the call as well
    with flux.Renderer(sd, flux.JobConfiguration(2, smooth_scenes.DEPTH, 50), seed=seed, set_share=(1, 2)) as share:
        share.set_mesh_normals(0, None)
        share.set_mesh_normals(0, sd.shapes[3].normals)


# ---- 7. the launch plan ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("root", smooth_scenes.ROOTS)
def test_launch_plan_and_device_bytes(flux, root):
    sd, seed, _ = smooth_scenes.reference("Matte", 2)
    with _renderer(flux, sd, root, seed) as r, _renderer(flux, smooth_scenes.flat_twin(sd), root, seed) as f:
        for math, kernel, trav in _configurations(flux):
            for x in (r, f):
                checks.configure(x, math, kernel, trav)
            # words 0-6 equal; word 7 too: no instantiation of its own (a wave-uniform branch on the table pointer), so no flag bit
            assert r.launch_plan(flags=True) == f.launch_plan(flags=True)
        assert r.device_bytes() == f.device_bytes() + 84 * 128   # one 128-B record per triangle of the scene
