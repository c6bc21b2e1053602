"""What the suites of the per-mesh attributes (corner normals: tests/test_gpu_smooth_normals.py; corner colours:
tests/test_gpu_vertex_colors.py) share: the configurations a mesh kernel runs in, one renderer per job, the quantities two contexts
are compared in, the feature-buffer comparison, the C client, and the bodies of the tests the two suites have in common.  A body
takes the suite's scenes module (tests/smooth_scenes.py, tests/color_scenes.py), its `twin` (the scene without the attribute) and
the attribute's MeshData field.  Below them, what the two suites without a GPU (tests/test_smooth_normals.py,
tests/test_vertex_colors.py) share.  Plain functions: each suite states its own scenes, seeds, tolerances and bad values."""
import ctypes as C
import dataclasses
import itertools
import os
import subprocess

import numpy as np
import pytest

import aov_spec
import extension_checks
import selftest
import smooth_scenes
import test_gpu_ext_fuzz as fuzz
from conftest import ROOT


def traversals(flux):
    return (flux._lib.TRAVERSE_BVH, flux._lib.TRAVERSE_BRUTE, flux._lib.TRAVERSE_BVH_BINARY)


def configurations(flux):
    return list(itertools.product((flux.MATH_FAST, flux.MATH_STRICT), (flux.KERNEL_DEFAULT, flux.KERNEL_STATIC, flux.KERNEL_REFILL),
                                  traversals(flux)))


def configure(r, math, kernel, trav):
    r.set_math(math)
    r.set_kernel(kernel)
    r.set_traversal(trav)


def renderer(flux, sd, root, seed, depth):
    return flux.Renderer(sd, flux.JobConfiguration(root, depth, 50), seed=seed)


def everything(r):
    """the five quantities two contexts are compared in: frame, statistics, feature buffers, chain buffers, moments"""
    r.enable_stats(True)
    r.stats(reset=True)
    frame = r.render_frame()
    return frame, r.stats(), r.render_aov(), r.render_aov_chain(), r.render_moments()


def assert_same(got, want, label):
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b if isinstance(a, dict) else np.array_equal(a, b, equal_nan=True), (label, k)


def assert_aov(got, want, label, tight):
    """`tight`: (channels, tolerance) pairs that hold besides aov_spec.TOL on every channel"""
    err = aov_spec.channel_errors(got, want)
    print(f"{label}: max |gpu - spec| per channel = " + " ".join(f"{e:.2e}" for e in err))
    assert got.shape == want.shape
    for channels, tol in tight:
        assert np.all(err[channels] <= tol), (label, err)
    assert np.all(err <= aov_spec.TOL), (label, err)
    assert np.array_equal(got[..., aov_spec.COVERAGE], want[..., aov_spec.COVERAGE]), label


# ---- the tests both suites have -------------------------------------------------------------------------------------------------

def debug_shade(flux, scenes, label, material):
    """scenes.debug_reference's rays: radiance within check_run's tolerances, t equal to rounding"""
    sd, seed, _ = scenes.reference(material, 2)
    o, d, set_index, index, rad, t_ref, _ = scenes.debug_reference(material)
    assert len(o) == smooth_scenes.DEBUG_RAYS
    with renderer(flux, sd, 2, seed, scenes.DEPTH) as r:
        for math, trav in itertools.product((flux.MATH_FAST, flux.MATH_STRICT), traversals(flux)):
            r.set_math(math)
            r.set_traversal(trav)
            rgb, hit, t = r.debug_shade(o, d, 1, set_index, index)
            assert np.array_equal(hit >= 0, np.isfinite(t_ref))
            on = hit >= 0
            assert np.max(np.abs(t[on] - t_ref[on]) / t_ref[on]) <= 1e-12
            err = np.abs(rgb - rad)
            print(f"{label} debug_shade {material} math {math} traversal {trav}: max {err.max():.3e}, 99.9th percentile {np.percentile(err, 99.9):.3e}")
            assert np.isfinite(rgb).all() and err.max() < fuzz.TOL and np.percentile(err, 99.9) < fuzz.TOL_TIGHT


def every_consumer(flux, scenes, twin, root, channels, shape_index, least, text):
    """Moments, the adaptive sampler and the three forms of render_denoised agree with the frame and the feature buffers of the
    context with the attribute; at root 2 the feature channels `channels` differ by more than `least` from the twin's on the pixels
    that shape `shape_index` covers alone"""
    sd, seed, spec = scenes.reference("Matte", 2)
    with renderer(flux, sd, root, seed, scenes.DEPTH) as r:
        r.set_kernel(flux.KERNEL_STATIC)   # channels 0..2 are the static kernel's frame bit for bit (tests/test_gpu_moments.py)
        frame, mom = r.render_frame(), r.render_moments()
        assert mom[..., :3].tobytes() == frame.tobytes()
        r.set_kernel(flux.KERNEL_DEFAULT)
        got, passes = r.render_adaptive(threshold=0.0, max_passes=1)
        assert got.tobytes() == mom.tobytes() and np.all(passes == 1)
        aov = r.render_aov()
        assert np.array_equal(r.render_denoised(variance="measured"), flux.denoise_moments(mom, aov), equal_nan=True)
        assert np.array_equal(r.render_denoised(), flux.denoise(r.render_frame(), aov), equal_nan=True)
        assert np.array_equal(r.render_denoised(guides="chain"), flux.denoise(r.render_frame(), r.render_aov_chain()), equal_nan=True)
    if root == 2:
        with renderer(flux, twin(sd), root, seed, scenes.DEPTH) as f:
            twin_aov = f.render_aov()
        covered = (spec.first_hits()[0] == shape_index).all(axis=2)
        assert covered.any()
        delta = np.abs(aov[..., channels] - twin_aov[..., channels])[covered]
        print(f"{text}: max {delta.max():.3f}")
        assert delta.max() > least   # the guides really change


def shares(flux, scenes, twin):
    """Set shares, row tiles and loopback ranks give the renderer's frame, which is not the twin's; the one-call multi render, which
    has no context to set an attribute on, refuses the scene"""
    sd, seed, _ = scenes.reference("Glossy", 2)
    cfg = flux.JobConfiguration(8, scenes.DEPTH, 50)
    with flux.Renderer(sd, cfg, seed=seed) as r:
        frame = r.render_frame()
        for world in (2, 3):
            assert np.array_equal(extension_checks.set_sharded_frame(flux, r, world).numpy(), frame)
        for step in (1, 4):
            assert np.array_equal(extension_checks.row_tiles(r, step), frame)
    for G, mode, got in extension_checks.loopback_frames(flux, sd, cfg, seed, (2, 3), (flux.SHARD_SETS, flux.SHARD_ROWS)):
        assert np.array_equal(got, frame), (G, mode)
    with flux.Renderer(twin(sd), cfg, seed=seed) as f:
        assert not np.array_equal(f.render_frame(), frame)
    with pytest.raises(flux.FluxError):
        flux.render_frame_multi(sd, cfg, seed=seed, num_devices=1)


def common_refusals(flux, r, attr, good):
    """The refusals every attribute call shares, on renderer `r` of a suite's scene (meshes of 80, 2 and 2 triangles) with `good`
    [80][3][3]: mesh out of range, wrong count, the other mesh's count, null pointer.  Returns refusal(mesh, array, count): the raw
    call, asserted to return FLUX_E_INVALID, and its message -- for the suite's own bad values."""
    call = getattr(flux._lib.lib, f"flux_ctx_set_mesh_{attr}")

    def refusal(mesh, arr, count):
        ptr = None if arr is None else arr.ctypes.data_as(flux._lib.C.POINTER(flux._lib.C.c_double))
        assert call(r._handle(), mesh, ptr, count) == flux._lib.E_INVALID
        return flux._lib.last_error()

    for mesh, arr, count, needle in ((3, good, 80, "mesh 3 out of range (3 meshes)"), (0, good, 79, f"mesh 0 has 80 triangles, got {attr} for 79"),
                                     (1, good, 80, "mesh 1 has 2 triangles"), (0, None, 80, "null pointer")):
        message = refusal(mesh, arr, count)
        assert needle in message, message
    return refusal


# ---- the C ABI from plain C -----------------------------------------------------------------------------------------------------

def fnv1a(data):
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def c_client(flux, tmp_path, name, scenes, twin, before, after):
    """tests/<name>.c built and run: its refusals went as the header says, and its three hashes are those of the frames the Python
    binding renders of scenes.c_client_scene with the attribute (`after`) and of its twin (`before`, and "cleared")"""
    exe = str(tmp_path / name)
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", name + ".c"), "-o", exe, "-L" + os.path.join(ROOT, "flux_amd"), "-lflux_hip", "-lm",
                    "-Wl,-rpath," + os.path.join(ROOT, "flux_amd"), "-Wl,-rpath,/opt/rocm/lib"], check=True)
    p = subprocess.run([exe, "8", "11"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr + p.stdout
    lines = dict(line.split(" ", 1) for line in p.stdout.splitlines())
    assert lines["refusals"] == "ok"
    sd = scenes.c_client_scene(flux)
    with flux.Renderer(sd, flux.JobConfiguration(8, 4, 50), seed=11) as r:
        with_attr = r.render_frame()
    with flux.Renderer(twin(sd), flux.JobConfiguration(8, 4, 50), seed=11) as r:
        without = r.render_frame()
    assert lines[after] == f"{fnv1a(with_attr.tobytes()):016x}"
    assert lines[before] == lines["cleared"] == f"{fnv1a(without.tobytes()):016x}"
    assert lines[after] != lines[before]


# ---- without a GPU: the loader, the entry point without a device, the host half stand-alone -------------------------------------

MESH_YAML = """
scene_name: t
camera_settings: {eye: [0, 1, -5], look_at: [0, 0, 0], up: [0, 1, 0]}
camera_data: {zoom_factor: 1.0, view_plane_distance: 500.0, focal_distance: 5.0, lens_radius: 0.0}
output_settings: {image_width: 4, image_height: 3, pixel_size: 50.0}
background: [0, 0, 0]
shapes:
  - Mesh:
      vertices: [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]]
      triangles: [[0, 1, 2], [0, 2, 3]]
      ATTRIBUTES
      material: {Matte: {diffuse_color: [1, 1, 1], ambient_color: [0, 0, 0], diffuse_coefficient: 1.0}}
"""


def load(flux, attribute_lines):
    """MESH_YAML's scene, a quad of two triangles, with the given lines in its Mesh block"""
    import yaml
    return flux.scene.scene_from_dict(yaml.safe_load(MESH_YAML.replace("ATTRIBUTES", attribute_lines)))


def loader_refusal(flux, line, message):
    with pytest.raises(flux.SceneError) as e:
        load(flux, line)
    assert message in str(e.value), str(e.value)


def meshdata_refusals(flux, attr, bad, message):
    """corner_<attr> of the quad refuses a wrong shape, a non-numeric entry, and the suite's `bad` value with `message`"""
    corners = getattr(flux.scene, f"corner_{attr}")
    mesh = load(flux, "").shapes[0]
    for value, needle in ((np.zeros((5, 3)), "expected [4][3] (per vertex) or [2][3][3] (per corner), got shape (5, 3)"),
                          (np.ones((3, 3, 3)), "got shape (3, 3, 3)"),
                          ([["a", 0, 1]] * 4, "expected numbers"),
                          (bad, message)):
        with pytest.raises(flux.SceneError) as e:
            corners(dataclasses.replace(mesh, **{attr: value}), "mesh 0")
        assert needle in str(e.value), str(e.value)
    return mesh


def null_context_refused(flux, attr):
    call = getattr(flux._lib.lib, f"flux_ctx_set_mesh_{attr}")
    n = (C.c_double * 9)(0, 0, 1, 0, 0, 1, 0, 0, 1)
    assert call(None, 0, n, 1) == flux._lib.E_INVALID
    assert "null context" in flux._lib.last_error()
    assert call(None, 0, None, 0) == flux._lib.E_INVALID


def host_selftest(tmp_path, name, check, sanitized):
    """tests/<name>.cpp built (with the sanitizers if `sanitized`) and run stand-alone; `check` judges its output"""
    if sanitized:
        exe = selftest.build(str(tmp_path / (name + "_san")), name + ".cpp", flags=selftest.SANITIZE)
        check(selftest.run(exe, env=selftest.sanitize_env()))
    else:
        check(selftest.run(selftest.build(str(tmp_path / name), name + ".cpp")))
