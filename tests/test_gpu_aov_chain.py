"""The feature buffers at the first non-specular hit on the GPU (flux_render_aov_chain_rows*) against their
specification in numpy (tests/aov_chain_spec.py; its cases are held to their margins and classes on the CPU by
tests/test_aov_chain.py): parity in both arithmetics, the three identities that tie the kernel to aov_kernel and to the render
kernels, the calls, the absence of side effects, the denoisers end to end and the command-line tool.

All scenes are 16 x 12 at seed 7 and depth 5.  Tolerance: aov_spec.TOL -- |Δ| <= 1e-9 on channels 0-5 and 7, |Δ| <= 1e-9 max(1, depth)
on depth, every pixel; coverage exact.  The spec folds in STRICT's order; FAST multiplies the same factors front to back, a few ulps
of values below 10.  No pixel is excluded: every decision of every case has a margin of at least 1e-9 (tests/test_aov_chain.py)."""
import os

import numpy as np
import pytest

import aov_chain_spec as cs
import aov_spec
import denoise_moments_spec as dms
import moments_spec
import path_spec
from conftest import small_scene
from extension_checks import cli_frame, host_bins, math_mode, small_yaml
from test_aov_chain import kept_pixels

pytestmark = pytest.mark.gpu

MATHS = ("fast", "strict")
SCENES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scenes")
CASE_IDS = [(name, root) for name, (_, roots, _) in cs.CASES.items() for root in roots]
_refs = {}


def reference(flux, name, root, max_chain=0):
    """(scene, spec buffers), computed once per (case, root, max_chain) and shared, read-only."""
    key = (name, root, max_chain)
    if key not in _refs:
        spec = cs.case_spec(flux, name, root)
        try:
            chain = cs.chain_buffers(spec, max_chain)
        finally:
            spec.close()
        chain.buffers.setflags(write=False)
        _refs[key] = (spec.sd, chain.buffers)
    return _refs[key]


def renderer(flux, sd, root, math="fast", traversal=None, depth=cs.DEPTH, **kw):
    r = flux.Renderer(sd, flux.JobConfiguration(root, depth, 50), seed=cs.SEED, **kw)
    r.set_math(math_mode(flux, math))
    if traversal is not None:
        r.set_traversal(traversal)
    return r


# ---- 1. the kernel against the spec -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("name,root", CASE_IDS, ids=[f"{n}-{r}" for n, r in CASE_IDS])
def test_parity_with_the_spec(flux, name, root, math):
    """Lane groups of 4 and 9 lanes, a whole wave, two chunks with 100 samples; the copy with the dielectric lobe (glass, box_room);
    box faces as chain vertices; partly covered pixels in every case, so in every copy; the TRIS instantiation in the three traversals, bit-equal; a FAST context routed to STRICT."""
    sd, want = reference(flux, name, root)
    L = flux._lib
    traversals = (("bvh", L.TRAVERSE_BVH), ("brute", L.TRAVERSE_BRUTE), ("binary", L.TRAVERSE_BVH_BINARY)) if name == "mesh" else (("", None),)
    frames = []
    for label, mode in traversals:
        with renderer(flux, sd, root, math, mode) as r:
            got = r.render_aov_chain()
            if name == "nonunit" and math == "fast":
                assert r.launch_plan()["math"] == L.MATH_STRICT
        aov_spec.assert_close(got, want, f"chain {name} root {root} {math} {label}")
        cov = got[..., aov_spec.COVERAGE]
        assert np.array_equal(cov, want[..., aov_spec.COVERAGE])
        assert ((cov > 0) & (cov < 1)).any()  # every case has an open sky: misses, fold(background), a depth mean over fewer than N
        frames.append(got)
    for other in frames[1:]:
        assert np.array_equal(frames[0], other, equal_nan=True)


@pytest.mark.parametrize("math", MATHS)
def test_a_chain_limit_of_two(flux, math):
    sd, want = reference(flux, "mirrors", 3, 2)
    with renderer(flux, sd, 3, math) as r:
        got = r.render_aov_chain(2)
    aov_spec.assert_close(got, want, f"chain mirrors root 3 {math} max_chain 2")
    assert np.array_equal(got[..., aov_spec.COVERAGE], want[..., aov_spec.COVERAGE])


# ---- 2. the identities ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("name,root", [("mirrors", 2), ("mirrors", 3), ("mirrors", 10), ("mesh", 8), ("glass", 4), ("box_room", 4)])
def test_max_chain_one_is_render_aov_bit_for_bit(flux, name, root, math):
    """In the three copies: STRICT, FAST, and FAST with the dielectric lobe (glass), whose first-hit pass runs the FAST copy."""
    sd = cs.CASES[name][0](flux)
    with renderer(flux, sd, root, math) as r:
        assert np.array_equal(r.render_aov_chain(1), r.render_aov(), equal_nan=True)


@pytest.mark.parametrize("math", MATHS)
def test_a_delta_free_scene_is_render_aov_bit_for_bit(flux, math):
    with renderer(flux, cs.delta_free_scene(flux), 3, math) as r:
        first = r.render_aov()
        for K in (0, 3):
            assert np.array_equal(r.render_aov_chain(K), first, equal_nan=True)


@pytest.mark.parametrize("root", [3, 16])
def test_all_emissive_terminals_give_the_render(flux, root):
    """The albedo carries the chain's throughput: where every non-specular material is Emissive (none brighter than 1, so max_to_one
    leaves the frame alone) it is the frame's unclamped mean.  Against render_frame() of the static, refill and split kernels on the
    pixels the CPU test keeps: within 1e-12 at root 3, bit for bit at root 16, where the three requests must plan three kernels
    (below 64 samples every request runs the static kernel, so root 3 compares with that one alone).  The scene's colours are dyadic:
    a pixel's sum is exact in any order, so neither bound can see a summation or fold order -- what is left at root 3 is this pass's
    division by 9 against the render's multiplication by 1/9 (measured 1.1e-16) --; what the test can see is a sample that took
    another bounce, another weight or another end than the render's."""
    sd = cs.mirror_emissive_scene(flux)
    spec = path_spec.PathSpec(sd, root, cs.DEPTH, cs.SEED)
    try:
        keep = kept_pixels(cs.chain_buffers(spec, 0))
    finally:
        spec.close()
    L = flux._lib
    with renderer(flux, sd, root) as r:
        alb = r.render_aov_chain()[..., aov_spec.ALBEDO]
        assert alb[keep].max() <= 1.0
        errs = {}
        for kernel, plan in ((flux.KERNEL_STATIC, L.PLAN_STATIC), (flux.KERNEL_REFILL, L.PLAN_REFILL), (flux.KERNEL_SPLIT, L.PLAN_SPLIT)):
            r.set_kernel(kernel)
            assert r.launch_plan()["kernel"] == (plan if root == 16 else L.PLAN_STATIC)
            frame = r.render_frame()
            errs[kernel] = (float(np.max(np.abs(frame[keep] - alb[keep]))), int(np.count_nonzero(frame[keep] != alb[keep])))
            print(f"chain emissive root {root} kernel {kernel} (plan {r.launch_plan()['kernel']}): max |render - albedo| = {errs[kernel][0]:.2e}, "
                  f"{errs[kernel][1]} values differ on {np.count_nonzero(keep)} pixels")
        for kernel, (err, differ) in errs.items():
            assert (differ == 0) if root == 16 else (err <= 1e-12), (kernel, err, differ)


# ---- 3. calls ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("root", [3, 8])
def test_row_tiles_strided_rows_and_refusals(flux, root):
    import torch
    sd = cs.mirror_scene(flux)
    L = flux._lib
    H, W = cs.H, cs.W
    with renderer(flux, sd, root) as r:
        frame = r.render_aov_chain()
        assert frame.shape == (H, W, 8)
        assert np.array_equal(r.render_aov_chain(), frame, equal_nan=True)  # run to run
        tiles = np.concatenate([r.render_aov_chain(0, a, min(a + 5, H) - 1) for a in range(0, H, 5)], axis=0)
        assert np.array_equal(tiles, frame, equal_nan=True)
        rows = list(range(1, H, 2))
        stream = torch.cuda.Stream()
        buf = torch.full((len(rows) + 2, W, 8), -7.0, dtype=torch.float64, device="cuda:0")  # a guard row on either side
        inner = buf[1:-1]
        torch.cuda.synchronize()
        r.render_aov_chain_device(1, 2, len(rows), inner.data_ptr(), 0, stream.cuda_stream)
        stream.synchronize()
        assert np.array_equal(inner.cpu().numpy(), frame[rows], equal_nan=True)
        assert bool((buf[0] == -7.0).all()) and bool((buf[-1] == -7.0).all())
        assert r.last_kernel_ms() > 0.0  # the launch sits between the context's two events
        buf.fill_(-7.0)
        torch.cuda.synchronize()
        r.render_aov_chain_device(0, 1, 0, inner.data_ptr())  # num_rows = 0: a no-op
        r.render_aov_chain_device(0, 1, 0, 0)
        torch.cuda.synchronize()
        assert bool((buf == -7.0).all())
        one_row = r.render_aov_chain(0, 4, 4)  # a one-row call after a frame-sized one
        for bad, words in ((lambda: r.render_aov_chain(0, 0, H), "rows"), (lambda: r.render_aov_chain(cs.DEPTH + 1), "max_chain 6 exceeds"),
                           (lambda: r.render_aov_chain_device(H, 1, 1, inner.data_ptr()), "rows"),
                           (lambda: r.render_aov_chain_device(H - 2, 2, 2, inner.data_ptr()), "rows"),
                           (lambda: r.render_aov_chain_device(0, 0, 1, inner.data_ptr()), "row_stride must be >= 1"),
                           (lambda: r.render_aov_chain_device(0, 1, 1, 0), "null output pointer"),
                           (lambda: r.render_aov_chain_device(0, 1, 1, inner.data_ptr(), cs.DEPTH + 1), "max_chain 6 exceeds the job's max_trace_depth 5")):
            with pytest.raises(flux.FluxError, match=words) as e:
                bad()
            assert e.value.code == L.E_INVALID
    with renderer(flux, sd, root) as fresh:  # a fresh context
        assert np.array_equal(fresh.render_aov_chain(0, 4, 4), one_row, equal_nan=True)
        assert np.array_equal(fresh.render_aov_chain(), frame, equal_nan=True)
    with renderer(flux, sd, root, set_share=(1, 2)) as part:
        with pytest.raises(flux.FluxError, match="sample sets") as e:
            part.render_aov_chain()
        assert e.value.code == L.E_INVALID


def test_a_strict_job_at_depth_40_gets_the_moments_refusal(flux):
    sd = cs.mirror_scene(flux)
    with renderer(flux, sd, 2, "strict", depth=40) as r:
        with pytest.raises(flux.FluxError, match="LDS per block") as want:
            r.render_moments()
        with pytest.raises(flux.FluxError, match="LDS per block") as got:
            r.render_aov_chain()
        assert got.value.code == want.value.code == flux._lib.E_INVALID
        assert "flux_render_aov_chain_rows" in str(got.value)


# ---- 4. no side effects -----------------------------------------------------------------------------------------------------------

def test_no_side_effects(flux):
    sd = cs.mirror_scene(flux)
    with renderer(flux, sd, 8) as r:
        r.enable_stats(True)
        r.stats(reset=True)
        plan = r.launch_plan()
        before = r.render_frame()
        stats = r.stats()
        assert stats["samples"] == cs.W * cs.H * 64
        aov, mom = r.render_aov(), r.render_moments()
        chain = r.render_aov_chain()
        assert r.stats() == stats        # the kernel keeps no statistics
        assert r.launch_plan() == plan
        r.stats(reset=True)
        after = r.render_frame()
        assert np.array_equal(before, after, equal_nan=True) and r.stats() == stats
        assert np.array_equal(r.render_aov(), aov, equal_nan=True) and np.array_equal(r.render_moments(), mom, equal_nan=True)
        assert np.array_equal(r.render_aov_chain(), chain, equal_nan=True)


# ---- 5. end to end ------------------------------------------------------------------------------------------------------------------

def test_denoisers_take_the_chain_buffer(flux):
    """denoise_moments(render_moments(), render_aov_chain()) against the two specs composed -- the moments of PathSpec's samples and
    the chain spec's buffers through tests/denoise_moments_spec.py --, and render_denoised(guides="chain") against the same."""
    sd = cs.mirror_scene(flux)
    spec = path_spec.PathSpec(sd, 3, cs.DEPTH, cs.SEED)
    try:
        chain = cs.chain_buffers(spec, 0).buffers
        spec.frame()
        mom = moments_spec.from_samples(spec.sample_radiance)
    finally:
        spec.close()
    want = dms.denoise_moments(mom, chain)
    with renderer(flux, sd, 3, "strict") as r:
        got = flux.denoise_moments(r.render_moments(), r.render_aov_chain())
        both = r.render_denoised(variance="measured", guides="chain")
        first = r.render_denoised(variance="measured")
        assert np.array_equal(first, r.render_denoised(variance="measured", guides="first"), equal_nan=True)
        assert np.array_equal(r.render_denoised(guides="chain"), flux.denoise(r.render_frame(), r.render_aov_chain()), equal_nan=True)
        with pytest.raises(flux.FluxError, match="guides") as e:
            r.render_denoised(guides="second")
        assert e.value.code == flux._lib.E_INVALID
    ok = np.isfinite(want)
    err = float(np.max(np.abs(got[ok] - want[ok])))
    print(f"denoise_moments over chain guides: max |gpu - specs composed| = {err:.2e}")
    assert np.array_equal(np.isfinite(got), ok) and err <= 1e-9
    assert np.array_equal(both, got, equal_nan=True)
    assert not np.array_equal(first, got, equal_nan=True)


def test_cli_writes_the_four_chain_buffers(flux, tmp_path):
    flux_bin, _ = host_bins()
    scene = small_yaml(os.path.join(SCENES, "mirror_glass.yml"), tmp_path, cs.W, cs.H)
    out = tmp_path / "out"
    cli_frame(flux_bin, scene, ["-r", "4", "--seed", "5", "--aov-chain", "0"], out)
    sd = flux.load_scene(scene)
    with flux.Renderer(sd, flux.JobConfiguration(4, 5, 50), seed=5) as r:
        chain = r.render_aov_chain()
        assert not np.array_equal(chain, r.render_aov(), equal_nan=True)
    kinds = ("albedo", "normal", "depth", "coverage")
    assert sorted(os.listdir(out)) == sorted([sd.scene_name + ".ppm"] + [f"{sd.scene_name}.chain_{k}.ppm" for k in kinds])
    for kind in kinds:
        want = tmp_path / f"want.{kind}.ppm"
        flux.write_ppm(str(want), aov_spec.aov_image(chain, kind))
        assert open(out / f"{sd.scene_name}.chain_{kind}.ppm", "rb").read() == open(want, "rb").read(), kind


@pytest.mark.parametrize("variance", ["spatial", "measured"])
def test_cli_denoises_with_chain_guides(flux, tmp_path, variance):
    flux_bin, _ = host_bins()
    scene = small_yaml(os.path.join(SCENES, "mirror_glass.yml"), tmp_path, cs.W, cs.H)
    sd = flux.load_scene(scene)
    with flux.Renderer(sd, flux.JobConfiguration(2, 5, 50), seed=7) as r:
        flux.write_ppm(str(tmp_path / "chain.ppm"), r.render_denoised(variance=variance, guides="chain"))
        flux.write_ppm(str(tmp_path / "first.ppm"), r.render_denoised(variance=variance))
    want = open(tmp_path / "chain.ppm", "rb").read()
    assert want != open(tmp_path / "first.ppm", "rb").read()
    cli_frame(flux_bin, scene, ["-r", "2", "--seed", "7", "--denoise", "--denoise-variance", variance, "--denoise-guides", "chain"], tmp_path / "out")
    assert sorted(os.listdir(tmp_path / "out")) == sorted([sd.scene_name + ".ppm", sd.scene_name + ".denoised.ppm"])
    assert open(tmp_path / "out" / (sd.scene_name + ".denoised.ppm"), "rb").read() == want
    cli_frame(flux_bin, scene, ["-r", "2", "--seed", "7", "--denoise", "--denoise-variance", variance, "--denoise-guides", "first"], tmp_path / "first")
    assert open(tmp_path / "first" / (sd.scene_name + ".denoised.ppm"), "rb").read() == open(tmp_path / "first.ppm", "rb").read()
