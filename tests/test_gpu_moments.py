"""The per-pixel sample moments on the GPU (flux_render_moments_rows*) against their specification in numpy
(tests/moments_spec.py over tests/path_spec.py's per-sample radiance): parity in both arithmetics and all three kernel copies, meshes
in the three traversals, the tie to the render kernels' frame, the calls, the refusals and the absence of side effects.

All scenes are 16 x 12 at seed 7, depth 5; tests/test_moments.py asserts on the CPU that each has noisy, zero-variance and clamped
pixels and no decision at rounding level.  Tolerance: 1e-9 absolute on channels 0-2 and 4-6 -- the project's bound for comparisons
with a spec --, and 1e-9 (ref + scale) on channels 3 and 7 with scale = m² for s2 and m² k² / N for var: the arithmetic differs by
~1e-13 relative (summation order, FMA in the FAST copies), while N for N - 1 moves every noisy pixel by 1 % or more."""
import numpy as np
import pytest

import moments_spec as ms
from conftest import small_scene
from extension_checks import math_mode

pytestmark = pytest.mark.gpu

MATHS = ("fast", "strict")
CASES = list(ms.CASES)


def gpu_moments(flux, sd, root, math, traversal=None, seed=ms.SEED, depth=ms.DEPTH):
    with flux.Renderer(sd, flux.JobConfiguration(root, depth, 50), seed=seed) as r:
        r.set_math(math_mode(flux, math))
        if traversal is not None:
            r.set_traversal(traversal)
        return r.render_moments()


# ---- 1. parity with the spec ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("name,root", CASES, ids=[f"{n}-{r}" for n, r in CASES])
def test_parity_with_the_spec(flux, name, root, math):
    """Lane groups of 4 (root 2) and of 9 lanes, which leave one lane of the wave idle (root 3); exactly one chunk (root 8); a
    partial second chunk (root 10); `glass` runs the copy with the dielectric lobe, `box_room` and `disk_light` the extension
    shapes, `open_mesh` the mesh instantiation."""
    sd, want, rad, _, _ = ms.reference(flux, name, root)
    got = gpu_moments(flux, sd, root, math)
    ms.assert_close(got, want, rad, f"{name} root {root} {math}")
    # the spec's conditions hold for the kernel's buffer too: the comparison above saw noisy and clamped pixels
    noisy, _, clamped = ms.counts(got, rad)
    assert (noisy, clamped) == (ms.CASES[(name, root)][0], ms.CASES[(name, root)][2])
    assert np.all(got[..., ms.S2] >= 0.0) and np.all(got[..., ms.VAR] >= 0.0)


# ---- 2. meshes ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("math", MATHS)
def test_meshes_in_the_three_traversals(flux, math):
    sd, want, rad, _, _ = ms.reference(flux, "open_mesh", 8)
    L = flux._lib
    frames = {}
    for name, mode in (("bvh", L.TRAVERSE_BVH), ("brute", L.TRAVERSE_BRUTE), ("binary", L.TRAVERSE_BVH_BINARY)):
        frames[name] = gpu_moments(flux, sd, 8, math, traversal=mode)
        ms.assert_close(frames[name], want, rad, f"open_mesh root 8 {math} {name}")
    assert np.array_equal(frames["bvh"], frames["brute"]) and np.array_equal(frames["bvh"], frames["binary"])


# ---- 3. the frame channels ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("root", [3, 10])
def test_frame_channels_are_the_static_kernels_frame(flux, root, math):
    sd = ms.scene(flux, "open")
    with flux.Renderer(sd, flux.JobConfiguration(root, ms.DEPTH, 50), seed=ms.SEED) as r:
        r.set_math(math_mode(flux, math))
        r.set_kernel(flux.KERNEL_STATIC)
        frame = r.render_frame()
        mom = r.render_moments()
    assert mom[..., ms.RGB].tobytes() == frame.tobytes()
    assert (mom[..., ms.MEAN].max(axis=2) > 1.0).any()  # max_to_one took part


def test_frame_channels_against_the_default_kernel(flux, demo2):
    sd = small_scene(demo2, ms.W, ms.H)
    with flux.Renderer(sd, flux.JobConfiguration(16, ms.DEPTH, 50), seed=ms.SEED) as r:
        frame = r.render_frame()
        assert r.launch_plan()["kernel"] != 0  # the default at 256 spp is not the static kernel
        mom = r.render_moments()
    err = float(np.abs(mom[..., ms.RGB] - frame).max())
    print(f"moments root 16: max |channels 0..2 - default kernel's frame| = {err:.2e}")
    assert err <= 1e-12


# ---- 4. calls, tiling and errors ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("root", [3, 8])
def test_row_tiles_strided_rows_and_refusals(flux, root):
    import torch
    sd = ms.scene(flux, "open")
    L = flux._lib
    with flux.Renderer(sd, flux.JobConfiguration(root, ms.DEPTH, 50), seed=ms.SEED) as r:
        frame = r.render_moments()
        assert frame.shape == (ms.H, ms.W, 8)
        tiles = np.concatenate([r.render_moments(a, min(a + 5, r.height) - 1) for a in range(0, r.height, 5)], axis=0)
        assert np.array_equal(tiles, frame)
        assert np.array_equal(r.render_moments(), frame)  # run to run
        rows = list(range(1, ms.H, 2))
        stream = torch.cuda.Stream(device="cuda:0")
        buf = torch.full((len(rows), ms.W, 8), -7.0, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        r.render_moments_device(1, 2, len(rows), buf.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        assert np.array_equal(buf.cpu().numpy(), frame[rows])
        assert r.last_kernel_ms() > 0.0  # the launch sits between the context's two events
        buf.fill_(-7.0)
        torch.cuda.synchronize()
        r.render_moments_device(0, 1, 0, buf.data_ptr(), stream=stream.cuda_stream)  # num_rows = 0: a no-op
        r.render_moments_device(0, 1, 0, 0)
        torch.cuda.synchronize()
        assert bool((buf == -7.0).all())
        for bad in (lambda: r.render_moments(0, ms.H), lambda: r.render_moments_device(ms.H, 1, 1, buf.data_ptr()),
                    lambda: r.render_moments_device(ms.H - 2, 2, 2, buf.data_ptr()), lambda: r.render_moments_device(0, 0, 1, buf.data_ptr()),
                    lambda: r.render_moments_device(0, 1, 1, 0)):
            with pytest.raises(flux.FluxError) as e:
                bad()
            assert e.value.code == L.E_INVALID
        assert np.array_equal(r.render_moments(), frame)  # the refusals left nothing behind
    with flux.Renderer(sd, flux.JobConfiguration(root, ms.DEPTH, 50), seed=ms.SEED, set_share=(1, 2)) as part:
        with pytest.raises(flux.FluxError, match="sample sets") as e:
            part.render_moments()
        assert e.value.code == L.E_INVALID


def test_one_sample_per_pixel_is_refused(flux):
    sd = ms.scene(flux, "open")
    with flux.Renderer(sd, flux.JobConfiguration(1, ms.DEPTH, 50), seed=ms.SEED) as r:
        with pytest.raises(flux.FluxError, match="no variance") as e:
            r.render_moments()
        assert e.value.code == flux._lib.E_INVALID and "flux_denoise" in str(e.value)
        with pytest.raises(flux.FluxError, match="no variance"):
            r.render_denoised(variance="measured")
        assert np.isfinite(r.render_frame()).all()


def test_a_strict_job_too_deep_for_the_static_kernels_lds_is_refused_like_its_render(flux, demo1):
    """40 levels * 32 B * 64 lanes > 64 KiB: the moments kernel keeps render_static_kernel's stacks, and is refused with its code."""
    sd = small_scene(demo1, ms.W, ms.H)
    with flux.Renderer(sd, flux.JobConfiguration(4, 40, 50), seed=ms.SEED) as r:
        r.set_math(flux.MATH_STRICT)
        r.set_kernel(flux.KERNEL_STATIC)
        with pytest.raises(flux.FluxError, match="64 KiB") as render:
            r.render_rows(0, 0)
        with pytest.raises(flux.FluxError, match="64 KiB") as moments:
            r.render_moments(0, 0)
        assert moments.value.code == render.value.code == flux._lib.E_INVALID
        assert "flux_render_moments_rows" in str(moments.value)
        r.set_math(flux.MATH_FAST)  # the context is usable afterwards
        assert np.isfinite(r.render_moments()).all()


# ---- 5. no side effects -----------------------------------------------------------------------------------------------------------

def test_no_side_effects(flux, demo2):
    sd = small_scene(demo2, ms.W, ms.H)
    with flux.Renderer(sd, flux.JobConfiguration(8, ms.DEPTH, 50), seed=ms.SEED) as r:
        r.enable_stats(True)
        r.stats(reset=True)
        plan = r.launch_plan()
        before = r.render_frame()
        stats = r.stats()
        assert stats["samples"] == ms.W * ms.H * 64
        mom = r.render_moments()
        assert r.stats() == stats        # the kernel keeps no statistics
        assert r.launch_plan() == plan
        r.stats(reset=True)
        after = r.render_frame()         # the host call's own buffer: the render's scratch framebuffer is untouched
        assert np.array_equal(before, after) and r.stats() == stats
        assert np.array_equal(r.render_moments(), mom)
        aov = r.render_aov()             # ... and so is the feature buffers'
        r.render_moments()
        assert np.array_equal(r.render_aov(), aov)
