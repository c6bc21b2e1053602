"""Adaptive sampling on the GPU (flux_render_adaptive_rows*, adaptive_body.inc, adaptive.hip) against its specification
in numpy (tests/adaptive_spec.py over tests/path_spec.py): parity in both arithmetics and all three kernel copies, meshes in the three
traversals, the calls, the state, the refusals, the absence of side effects, the denoiser behind it and the command-line tool.

The scenes are 16 x 12 at seed 7, depth 5, so S = 16, but for section 2b's frames of 41 x 27, 67 x 47 and 130 x 127 pixels, which fill
more than one selection block; tests/test_adaptive.py asserts on the CPU that no hot decision and no path decision of a case sits
at rounding level, so the pass map must be EQUAL.  The generated scenes: tests/test_gpu_pass_fuzz.py.  Tolerance on the eight channels: moments_spec's -- 1e-9
absolute on channels 0-2 and 4-6, 1e-9 (ref + scale) on channels 3 and 7 with scale = m² for s2 and m² k² / n for var, n = N c."""
import os

import numpy as np
import pytest

import adaptive_spec as asp
import denoise_moments_spec as dms
import moments_spec as ms
from conftest import SCENES, small_scene
from extension_checks import cli_frame, host_bins, math_mode, small_yaml
from path_spec import aov_buffers, PathSpec

pytestmark = pytest.mark.gpu

MATHS = ("fast", "strict")


def renderer(flux, sd, root, math="fast", traversal=None, depth=ms.DEPTH):
    r = flux.Renderer(sd, flux.JobConfiguration(root, depth, 50), seed=ms.SEED)
    r.set_math(math_mode(flux, math))
    if traversal is not None:
        r.set_traversal(traversal)
    return r


def gpu_adaptive(flux, sd, root, par, math="fast", traversal=None):
    with renderer(flux, sd, root, math, traversal) as r:
        mom, passes = r.render_adaptive(**par)
        return mom, passes, r.last_adaptive_info


# ---- 1. parity with the spec ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("name", list(asp.CASES) + list(asp.SPECIAL))
def test_parity_with_the_spec(flux, name, math):
    """16 pixels per wave (root 2) and 9-lane groups with one lane idle (root 3), whose lists are no multiple of the pixels per wave;
    exactly one chunk (root 8); a partial second chunk (root 10); `glass` runs the copy with the dielectric lobe, `box_room` and
    `disk_light` the extension shapes, `open_mesh` the mesh instantiation; `wrap-2` runs 16 passes so that the sets wrap past S;
    `single-3x2` ends on a list with ONE entry; `round1-2` stops at its first selection."""
    sd, par, want = asp.case(flux, name)
    root = (asp.CASES.get(name) or asp.SPECIAL[name])[1]
    got, passes, info = gpu_adaptive(flux, sd, root, par, math)
    asp.assert_close(got, passes, want, f"{name} {math}", root * root)
    assert info["rounds"] == len(want.active) and info["pixel_passes"] == int(want.passes.sum()) == int(passes.sum())
    assert info["pixels_at_max_passes"] == int(np.count_nonzero(want.passes == par["max_passes"]))
    assert info["samples"] == root * root * int(passes.sum())
    assert np.all(got[..., ms.S2] >= 0.0) and np.all(got[..., ms.VAR] >= 0.0)


@pytest.mark.parametrize("math", MATHS)
def test_meshes_in_the_three_traversals(flux, math):
    sd, par, want = asp.case(flux, "open_mesh-8")
    L = flux._lib
    runs = {}
    for name, mode in (("bvh", L.TRAVERSE_BVH), ("brute", L.TRAVERSE_BRUTE), ("binary", L.TRAVERSE_BVH_BINARY)):
        runs[name] = gpu_adaptive(flux, sd, 8, par, math, traversal=mode)
        asp.assert_close(runs[name][0], runs[name][1], want, f"open_mesh-8 {math} {name}", 64)
    for other in ("brute", "binary"):
        assert np.array_equal(runs["bvh"][0], runs[other][0]) and np.array_equal(runs["bvh"][1], runs[other][1])


# ---- 2. calls and state ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("name,root", [("open", 2), ("open", 3), ("open", 10), ("open_mesh", 8), ("glass", 4)])
def test_one_pass_is_the_sample_moments_bit_for_bit(flux, name, root, math):
    sd = ms.scene(flux, name)
    with renderer(flux, sd, root, math) as r:
        mom = r.render_moments()
        got, passes = r.render_adaptive(threshold=0.0, max_passes=1)
        assert got.tobytes() == mom.tobytes()
        assert np.all(passes == 1)
        assert r.last_adaptive_info == {"rounds": 1, "pixel_passes": ms.W * ms.H, "pixels_at_max_passes": ms.W * ms.H,
                                        "samples": ms.W * ms.H * root * root}
        # min_passes = max_passes = 3: no selection at all, every pixel three sets
        _, three = r.render_adaptive(threshold=1e9, min_passes=3, max_passes=3)
        assert np.all(three == 3) and r.last_adaptive_info["rounds"] == 3


@pytest.mark.parametrize("root", [2, 8])
def test_two_runs_and_row_tiles_are_bit_equal(flux, root):
    sd = ms.scene(flux, "open")
    par = dict(threshold=0.1 if root == 2 else 0.05, max_passes=5, dilate=0)
    with renderer(flux, sd, root) as r:
        mom, passes = r.render_adaptive(**par)
        assert len(np.unique(passes)) > 2
        again = r.render_adaptive(**par)
        assert np.array_equal(again[0], mom) and np.array_equal(again[1], passes)
        # with dilate = 0 a pixel depends on nothing but itself: tiles of 5 rows are the frame
        tiles = [r.render_adaptive(row_start=a, row_end=min(a + 5, r.height) - 1, **par) for a in range(0, r.height, 5)]
        assert np.array_equal(np.concatenate([t[0] for t in tiles], axis=0), mom)
        assert np.array_equal(np.concatenate([t[1] for t in tiles], axis=0), passes)
        # a smaller call after a larger one reuses the context's state buffers: no stale state
        one = r.render_adaptive(row_start=3, row_end=3, **par)
        assert np.array_equal(one[0], mom[3:4]) and np.array_equal(one[1], passes[3:4])
    with renderer(flux, sd, root) as fresh:   # ... and a fresh context computes the same
        other = fresh.render_adaptive(**par)
        assert np.array_equal(other[0], mom) and np.array_equal(other[1], passes)


def test_device_entry_on_a_stream_with_guard_bands(flux):
    import torch
    sd, par, want = asp.case(flux, "open-2")
    guard = 64
    with renderer(flux, sd, 2) as r:
        mom, passes = r.render_adaptive(**par)
        info = dict(r.last_adaptive_info)
        stream = torch.cuda.Stream(device="cuda:0")
        dmom = torch.full((ms.H * ms.W * 8 + guard,), -7.0, dtype=torch.float64, device="cuda:0")
        dmap = torch.full((ms.H * ms.W + guard,), 0x5a5a5a5a, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        r.render_adaptive_device(0, 1, ms.H, dmom.data_ptr(), dmap.data_ptr(), stream=stream.cuda_stream, **par)
        stream.synchronize()
        assert r.last_kernel_ms() > 0.0  # the call's launches sit between the context's two events
        assert r.last_adaptive_info == info
        hm, hp = dmom.cpu().numpy(), dmap.cpu().numpy()
        assert np.array_equal(hm[:-guard].reshape(ms.H, ms.W, 8), mom) and np.array_equal(hp[:-guard].reshape(ms.H, ms.W), passes.view(np.int32))
        assert np.all(hm[-guard:] == -7.0) and np.all(hp[-guard:] == 0x5a5a5a5a)
        # strided rows with dilate 0 are those rows of the frame's dilate-0 run; num_rows = 0 is a no-op
        par0 = dict(par, dilate=0)
        frame0 = r.render_adaptive(**par0)
        rows = list(range(1, ms.H, 2))
        dmom.fill_(-7.0)
        dmap.fill_(0x5a5a5a5a)
        torch.cuda.synchronize()
        r.render_adaptive_device(1, 2, len(rows), dmom.data_ptr(), dmap.data_ptr(), stream=stream.cuda_stream, **par0)
        stream.synchronize()
        k = len(rows) * ms.W
        assert np.array_equal(dmom.cpu().numpy()[:k * 8].reshape(len(rows), ms.W, 8), frame0[0][rows])
        assert np.array_equal(dmap.cpu().numpy()[:k].reshape(len(rows), ms.W), frame0[1][rows].view(np.int32))
        assert bool((dmom[k * 8:] == -7.0).all()) and bool((dmap[k:] == 0x5a5a5a5a).all())
        dmom.fill_(-7.0)
        torch.cuda.synchronize()
        r.render_adaptive_device(0, 1, 0, dmom.data_ptr(), dmap.data_ptr(), stream=stream.cuda_stream)
        r.render_adaptive_device(0, 1, 0, 0, 0)
        torch.cuda.synchronize()
        assert bool((dmom == -7.0).all())
        assert r.last_adaptive_info == {"rounds": 0, "pixel_passes": 0, "pixels_at_max_passes": 0, "samples": 0}


def test_refusals_that_need_a_context(flux):
    sd = ms.scene(flux, "open")
    L = flux._lib
    with renderer(flux, sd, 2) as r:
        frame = r.render_adaptive(threshold=0.2, max_passes=4)
        for bad, word in ((lambda: r.render_adaptive(max_passes=ms.W + 1), "sample sets"),
                          (lambda: r.render_adaptive(row_start=0, row_end=ms.H), "outside image height"),
                          (lambda: r.render_adaptive_device(ms.H, 1, 1, 0x1000, 0x1000), "exceed image height"),
                          (lambda: r.render_adaptive_device(ms.H - 2, 2, 2, 0x1000, 0x1000), "exceed image height"),
                          (lambda: r.render_adaptive_device(0, 0, 1, 0x1000, 0x1000), "row_stride"),
                          (lambda: r.render_adaptive_device(0, 1, 1, 0, 0x1000), "null output"),
                          (lambda: r.render_adaptive_device(0, 1, 1, 0x1000, 0), "null output"),
                          (lambda: r.render_adaptive(threshold=-1.0), "threshold"),
                          (lambda: r.render_adaptive(dilate=3), "dilate")):
            with pytest.raises(flux.FluxError, match=word) as e:
                bad()
            assert e.value.code == L.E_INVALID
        assert r.render_adaptive(max_passes=ms.W, threshold=1e9)[1].max() == 1  # S itself is allowed
        again = r.render_adaptive(threshold=0.2, max_passes=4)  # the refusals left nothing behind
        assert np.array_equal(again[0], frame[0]) and np.array_equal(again[1], frame[1])
    with flux.Renderer(sd, flux.JobConfiguration(2, ms.DEPTH, 50), seed=ms.SEED, set_share=(1, 2)) as part:
        with pytest.raises(flux.FluxError, match="sample sets") as e:
            part.render_adaptive()
        assert e.value.code == L.E_INVALID
    with flux.Renderer(sd, flux.JobConfiguration(1, ms.DEPTH, 50), seed=ms.SEED) as one:
        with pytest.raises(flux.FluxError, match="no variance") as e:
            one.render_adaptive()
        assert e.value.code == L.E_INVALID
        assert np.isfinite(one.render_frame()).all()


def test_a_strict_job_too_deep_for_the_lds_is_refused_like_its_moments(flux, demo1):
    """40 levels * 32 B * 64 lanes > 64 KiB: the pass kernel keeps moments_kernel's stacks, and is refused with its code."""
    sd = small_scene(demo1, ms.W, ms.H)
    with flux.Renderer(sd, flux.JobConfiguration(4, 40, 50), seed=ms.SEED) as r:
        r.set_math(flux.MATH_STRICT)
        with pytest.raises(flux.FluxError, match="64 KiB") as moments:
            r.render_moments(0, 0)
        with pytest.raises(flux.FluxError, match="64 KiB") as adaptive:
            r.render_adaptive(row_start=0, row_end=0)
        assert adaptive.value.code == moments.value.code == flux._lib.E_INVALID
        assert "flux_render_adaptive_rows" in str(adaptive.value)
        r.set_math(flux.MATH_FAST)  # the context is usable afterwards
        assert np.isfinite(r.render_adaptive(max_passes=3)[0]).all()


def test_no_side_effects(flux, demo2):
    sd = small_scene(demo2, ms.W, ms.H)
    with flux.Renderer(sd, flux.JobConfiguration(4, ms.DEPTH, 50), seed=ms.SEED) as r:
        r.enable_stats(True)
        r.stats(reset=True)
        plan = r.launch_plan()
        before = r.render_frame()
        stats = r.stats()
        assert stats["samples"] == ms.W * ms.H * 16
        mom, aov = r.render_moments(), r.render_aov()
        got = r.render_adaptive(threshold=0.05, max_passes=4)
        assert got[1].max() > 1
        assert r.stats() == stats        # the kernels keep no statistics
        assert r.launch_plan() == plan
        r.stats(reset=True)
        after = r.render_frame()         # buffers of its own: no other call's scratch is touched
        assert np.array_equal(before, after) and r.stats() == stats
        assert np.array_equal(r.render_moments(), mom) and np.array_equal(r.render_aov(), aov)
        again = r.render_adaptive(threshold=0.05, max_passes=4)
        assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])


# ---- 2b. more than one selection block ------------------------------------------------------------------------------------------------
# adaptive_spec.BLOCK_CASES: scene `open` at 41 x 27, 67 x 47 and 130 x 127.  tests/test_adaptive.py asserts their margins and, from the
# reference alone, what each reaches in adaptive.hip: block bases that come from another block's atomic add, an empty selection block
# beside a non-empty one, blocks whose sixteen waves all hold an active pixel, a count kernel that strides.

@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("name", list(asp.BLOCK_CASES))
def test_parity_with_the_spec_beyond_one_selection_block(flux, name, math):
    sd, par, want = asp.case(flux, name)
    root = asp.BLOCK_CASES[name][1]
    got, passes, info = gpu_adaptive(flux, sd, root, par, math)
    asp.assert_close(got, passes, want, f"{name} {math}", root * root)
    assert info["rounds"] == len(want.active) and info["pixel_passes"] == int(want.passes.sum()) == int(passes.sum())
    assert info["pixels_at_max_passes"] == int(np.count_nonzero(want.passes == par["max_passes"]))
    assert info["samples"] == root * root * int(passes.sum())
    assert np.all(got[..., ms.S2] >= 0.0) and np.all(got[..., ms.VAR] >= 0.0)
    if name == "blocks-130x127-2":   # the count kernel's verdict on the map it was given, the spec aside
        assert passes.size > 64 * 256
        assert info["pixels_at_max_passes"] == int(np.count_nonzero(passes == par["max_passes"]))
        assert info["pixel_passes"] == int(passes.astype(np.int64).sum())


def test_strided_rows_with_dilation_against_the_spec(flux):
    """Rows 1, 3, ... 45 of the 67 x 47 frame with dilate 2 through the device entry on a non-default stream: 1541 pixels in two
    selection blocks, the neighbourhood in the call's LOCAL row index.  tests/test_adaptive.py asserts that the frame's own run gives
    another pass map on these rows."""
    import torch
    name = "blocks-67x47-3"
    w, h = asp.BLOCK_CASES[name][3]
    rows = np.arange(1, h, 2)
    sd, par, want = asp.rows_case(flux, name, rows)
    assert par["dilate"] == 2 and len(rows) == 23
    k, guard = len(rows) * w, 64
    with renderer(flux, sd, 3) as r:
        stream = torch.cuda.Stream(device="cuda:0")
        dmom = torch.full((k * 8 + guard,), -7.0, dtype=torch.float64, device="cuda:0")
        dmap = torch.full((k + guard,), 0x5a5a5a5a, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        r.render_adaptive_device(1, 2, len(rows), dmom.data_ptr(), dmap.data_ptr(), stream=stream.cuda_stream, **par)
        stream.synchronize()
        info = dict(r.last_adaptive_info)
        hm, hp = dmom.cpu().numpy(), dmap.cpu().numpy()
    assert np.all(hm[k * 8:] == -7.0) and np.all(hp[k:] == 0x5a5a5a5a)
    passes = hp[:k].reshape(len(rows), w).view(np.uint32)
    asp.assert_close(hm[:k * 8].reshape(len(rows), w, 8), passes, want, f"{name} rows 1, 3, ... 45", 9)
    assert info == {"rounds": len(want.active), "pixel_passes": int(want.passes.sum()), "samples": 9 * int(want.passes.sum()),
                    "pixels_at_max_passes": int(np.count_nonzero(want.passes == par["max_passes"]))}


def test_row_tiles_with_dilation_against_the_spec(flux):
    """Tiles of 10 rows of the 67 x 47 frame with dilate 1, each against the rule run over that tile's rows alone."""
    name = "blocks-67x47-3"
    w, h = asp.BLOCK_CASES[name][3]
    sd = asp.case(flux, name)[0]
    with renderer(flux, sd, 3) as r:
        for a in range(0, h, 10):
            rows = np.arange(a, min(a + 10, h))
            _, par, want = asp.rows_case(flux, name, rows, dilate=1)
            got, passes = r.render_adaptive(row_start=int(rows[0]), row_end=int(rows[-1]), **par)
            asp.assert_close(got, passes, want, f"{name} rows {rows[0]}..{rows[-1]} dilate 1", 9)
            assert r.last_adaptive_info["rounds"] == len(want.active) and r.last_adaptive_info["pixel_passes"] == int(want.passes.sum())


def test_one_context_through_calls_of_growing_and_shrinking_size(flux):
    """One row, the frame, five rows, the frame: d_adapt_pixels and d_adapt_out_pixels grow once, and the later calls find a list
    buffer that holds a longer, older list.  Each result is what a fresh context returns for the same call, bit for bit."""
    name = "blocks-41x27-2"
    sd, par, want = asp.case(flux, name)
    w, h = asp.BLOCK_CASES[name][3]
    calls = [(3, 3), (0, h - 1), (0, 4), (0, h - 1)]
    with renderer(flux, sd, 2) as r:
        got = [r.render_adaptive(row_start=a, row_end=b, **par) + (dict(r.last_adaptive_info),) for a, b in calls]
    for (a, b), (mom, passes, info) in zip(calls, got):
        with renderer(flux, sd, 2) as fresh:
            fmom, fpasses = fresh.render_adaptive(row_start=a, row_end=b, **par)
            assert mom.shape == (b - a + 1, w, 8) and fmom.tobytes() == mom.tobytes() and np.array_equal(fpasses, passes), (a, b)
            assert fresh.last_adaptive_info == info, (a, b)
    for k in (1, 3):
        asp.assert_close(got[k][0], got[k][1], want, f"{name} call {k + 1} of one context", 4)


# ---- 3. end to end --------------------------------------------------------------------------------------------------------------

def test_denoise_moments_filters_an_adaptive_frame(flux):
    """No new denoiser call: the output is the moments layout.  Within 1e-9 of the two specs composed."""
    sd, par, want = asp.case(flux, "open-2")
    spec = PathSpec(sd, 2, ms.DEPTH, ms.SEED)
    try:
        spec.frame()
        aov = aov_buffers(spec)
    finally:
        spec.close()
    with renderer(flux, sd, 2) as r:
        got = flux.denoise_moments(r.render_adaptive(**par)[0], r.render_aov())
        plain = flux.denoise_moments(r.render_moments(), r.render_aov())
    ref = dms.denoise_moments(want.moments, aov)
    err = float(np.abs(got - ref).max())
    print(f"denoise_moments over an adaptive frame: max |gpu - specs composed| = {err:.2e}")
    assert err <= 1e-9
    assert float(np.abs(got - plain).max()) > 1e-3  # the further passes reached the filter


def test_cli_writes_the_adaptive_frame_and_the_pass_map(flux, tmp_path):
    flux_bin, _ = host_bins()
    scene = small_yaml(os.path.join(SCENES, "demo2.yml"), tmp_path, 64, 48)
    sd = flux.load_scene(scene)
    with flux.Renderer(sd, flux.JobConfiguration(2, 5, 50), seed=7) as r:
        mom, passes = r.render_adaptive(threshold=0.1, max_passes=6)
        plain = r.render_moments()
    assert len(np.unique(passes)) > 2
    flux.write_ppm(str(tmp_path / "want.ppm"), np.ascontiguousarray(mom[..., ms.RGB]))
    flux.write_ppm(str(tmp_path / "plain.ppm"), np.ascontiguousarray(plain[..., ms.RGB]))
    grey = np.repeat((passes.astype(np.float64) / 6.0)[..., None], 3, axis=2)
    flux.write_ppm(str(tmp_path / "map.ppm"), np.ascontiguousarray(grey))
    want = open(tmp_path / "want.ppm", "rb").read()
    assert want != open(tmp_path / "plain.ppm", "rb").read()
    cli_frame(flux_bin, scene, ["-r", "2", "--seed", "7", "--adaptive", "0.1", "--adaptive-max-passes", "6"], tmp_path / "out")
    assert sorted(os.listdir(tmp_path / "out")) == sorted([sd.scene_name + ".ppm", sd.scene_name + ".adaptive.ppm", sd.scene_name + ".passes.ppm"])
    assert open(tmp_path / "out" / (sd.scene_name + ".adaptive.ppm"), "rb").read() == want
    assert open(tmp_path / "out" / (sd.scene_name + ".passes.ppm"), "rb").read() == open(tmp_path / "map.ppm", "rb").read()
