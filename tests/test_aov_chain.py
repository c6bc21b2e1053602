"""The feature buffers at the first non-specular hit without a GPU: the specification itself (tests/aov_chain_spec.py)
on the cases the kernel is then held to (tests/test_gpu_aov_chain.py) -- the margins of its decisions, the classes its chains reach and
its three identities --, the argument checks of the two entry points that need no context, flux_host::render_aov_chain's refusals (also
as a stand-alone program under the address and undefined-behaviour sanitizers), and the command-line tool's refusals.

Every case has an open sky (`glass` without its environment sphere, `box_room` with only the floor of its room), so every case has
partly covered pixels and misses behind bounces.  Counts measured when the scenes were chosen (root of the first column, max_chain 0;
chain-length classes 1, 2, 3, >= 4; cut at max_chain 2; partly covered pixels):
    mirrors  2   153  100  141  374     515   38                    glass     4  2070   67  878   57   935   53  (151 reflections, 1864 transmissions)
    mesh     8  3281 7923  760  324    1084   41                    box_room  4  1274  286 1307  205  1512   91  (245 reflections, 2978 transmissions)
    nonunit  3   343  298  319  768    1087   57"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aov_chain_spec as cs
import aov_spec
import path_spec
from conftest import ROOT, SCENES
import selftest
import switches
from extension_checks import host_bins

MARGIN = 1e-9
CASE_IDS = [(name, root) for name, (_, roots, _) in cs.CASES.items() for root in roots]


@pytest.fixture(scope="module")
def specs(flux):
    """(case, root) -> (PathSpec, Chain at max_chain 0), built once per module."""
    made = {}

    def get(name, root):
        if (name, root) not in made:
            spec = cs.case_spec(flux, name, root)
            made[name, root] = (spec, cs.chain_buffers(spec, 0))
        return made[name, root]
    yield get
    for spec, _ in made.values():
        spec.close()


def test_the_binding_has_the_calls(flux):
    hdr = open(os.path.join(ROOT, "include", "flux_abi.h")).read()
    assert "flux_render_aov_chain_rows(" in hdr and "flux_render_aov_chain_rows_device(" in hdr
    assert "#define FLUX_ABI_VERSION 3" in hdr
    for name in ("render_aov_chain", "render_aov_chain_device"):
        assert hasattr(flux.Renderer, name)


@pytest.mark.parametrize("name,root", CASE_IDS, ids=[f"{n}-{r}" for n, r in CASE_IDS])
def test_cases_reach_what_they_are_for(specs, name, root):
    spec, chain = specs(name, root)
    L = chain.length
    classes = [int((L == 1).sum()), int((L == 2).sum()), int((L == 3).sum()), int((L >= 4).sum())]
    cut2 = int(cs.chain_buffers(spec, 2).cut.sum())
    hits = chain.covered.sum(axis=2)
    partly = int(np.count_nonzero((hits > 0) & (hits < spec.N)))
    margin = min(chain.margins.values())
    print(f"{name}-{root}: classes {classes}, cut at 2: {cut2}, reflections {chain.reflections}, transmissions {chain.transmissions}, "
          f"mirror bounces {chain.mirror_bounces}, partly covered {partly}, smallest margin {margin:.2e}")
    assert margin >= MARGIN, chain.margins
    assert min(classes) >= 50, classes
    assert cut2 >= 20
    if cs.CASES[name][2]:
        assert chain.reflections >= 100 and chain.transmissions >= 100
    assert partly >= 1
    first = path_spec.aov_buffers(spec)
    d = np.abs(chain.buffers - first)
    with np.errstate(invalid="ignore"):
        differs = (d[..., aov_spec.ALBEDO].max(axis=2) > 1e-3) & (d[..., aov_spec.NORMAL].max(axis=2) > 1e-3) & (d[..., aov_spec.DEPTH] > 1e-3)
    assert differs.any()  # a pixel whose chain buffer is another one in albedo, in normal and in depth


@pytest.mark.parametrize("name,root", [("mirrors", 3), ("glass", 4), ("mesh", 8)])
def test_max_chain_one_is_the_first_hit_buffer(specs, name, root):
    spec, _ = specs(name, root)
    assert np.array_equal(cs.chain_buffers(spec, 1).buffers, path_spec.aov_buffers(spec))


def test_a_delta_free_scene_is_the_first_hit_buffer(flux):
    spec = path_spec.PathSpec(cs.delta_free_scene(flux), 3, cs.DEPTH, cs.SEED)
    try:
        first = path_spec.aov_buffers(spec)
        for K in (0, 3):
            chain = cs.chain_buffers(spec, K)
            assert np.array_equal(chain.buffers, first)
            assert int(chain.length.max()) == 1
    finally:
        spec.close()


def kept_pixels(chain):
    """The pixels none of whose samples ends on a delta material at k == K; at most a quarter may be left out."""
    keep = ~chain.cut.any(axis=2)
    assert np.count_nonzero(~keep) * 4 <= keep.size, np.count_nonzero(~keep)
    return keep


@pytest.mark.parametrize("root", [3, 16])
def test_all_emissive_terminals_give_the_radiance(flux, root):
    """Every non-specular material Emissive: a kept sample's folded albedo is PathSpec's radiance of the sample bit for bit, and so is
    the pixel's mean.  (Root 16 is the GPU test's bit-for-bit case; its cap on left-out pixels is counted here.)"""
    spec = path_spec.PathSpec(cs.mirror_emissive_scene(flux), root, cs.DEPTH, cs.SEED)
    try:
        chain = cs.chain_buffers(spec, 0)
        spec.frame()
        keep = kept_pixels(chain)
        print(f"root {root}: {np.count_nonzero(~keep)} of {keep.size} pixels left out as cut")
        assert np.array_equal(chain.albedo[keep], spec.sample_radiance[keep], equal_nan=True)
        mean = np.zeros(chain.albedo.shape[:2] + (3,))
        for i in range(spec.N):
            mean = mean + spec.sample_radiance[:, :, i]
        assert np.array_equal(chain.buffers[..., aov_spec.ALBEDO][keep], (mean / spec.N)[keep], equal_nan=True)
        assert min(chain.margins.values()) >= MARGIN
    finally:
        spec.close()


def test_spec_refuses_a_chain_beyond_the_depth(flux):
    spec = path_spec.PathSpec(cs.delta_free_scene(flux), 2, 3, cs.SEED)
    try:
        with pytest.raises(ValueError, match="max_chain 4 exceeds max_trace_depth 3"):
            cs.chain_buffers(spec, 4)
    finally:
        spec.close()


# ---- the entry points' checks that need no context ------------------------------------------------------------------------------

def test_entry_points_refuse_without_reading_the_context(flux):
    """A context pointer that must never be dereferenced: address 8 is no object."""
    L = flux._lib
    lib, ctx = L.lib, C.c_void_p(8)
    out = (C.c_double * 8)()
    checks = [
        (lambda: lib.flux_render_aov_chain_rows(None, 0, 0, 0, out), "flux_render_aov_chain_rows: null context"),
        (lambda: lib.flux_render_aov_chain_rows(ctx, 0, 0, 0, None), "flux_render_aov_chain_rows: null output pointer"),
        (lambda: lib.flux_render_aov_chain_rows(ctx, 0, 0, 257, out), "flux_render_aov_chain_rows: max_chain 257 exceeds 256"),
        (lambda: lib.flux_render_aov_chain_rows(ctx, 3, 2, 0, out), "flux_render_aov_chain_rows: row_end 2 is below row_start 3"),
        (lambda: lib.flux_render_aov_chain_rows_device(None, 0, 1, 1, 0, C.c_void_p(8), None), "flux_render_aov_chain_rows_device: null context"),
        (lambda: lib.flux_render_aov_chain_rows_device(ctx, 0, 1, 1, 0, None, None), "flux_render_aov_chain_rows_device: null output pointer"),
        (lambda: lib.flux_render_aov_chain_rows_device(ctx, 0, 1, 1, 300, C.c_void_p(8), None),
         "flux_render_aov_chain_rows_device: max_chain 300 exceeds 256"),
        (lambda: lib.flux_render_aov_chain_rows_device(ctx, 0, 0, 1, 0, C.c_void_p(8), None),
         "flux_render_aov_chain_rows_device: row_stride must be >= 1"),
    ]
    for call, message in checks:
        assert call() == L.E_INVALID, message
        assert L.last_error().startswith(message), (L.last_error(), message)


def test_python_refuses_unknown_guides_and_a_max_chain_outside_32_bits(flux):
    class Stub(flux.Renderer):
        def __init__(self):
            pass

        def __del__(self):
            pass
    with pytest.raises(flux.FluxError, match="guides must be 'first' or 'chain'"):
        flux.Renderer.render_denoised(Stub(), guides="second")
    for call in (lambda v: flux.Renderer.render_aov_chain(Stub(), v, 0, 0), lambda v: flux.Renderer.render_aov_chain_device(Stub(), 0, 1, 1, 8, v)):
        for value in (-1, 2 ** 32, 2 ** 32 + 3):  # (a uint32_t parameter would wrap the last two to 0 and 3)
            with pytest.raises(flux.FluxError, match="max_chain") as e:
                call(value)
            assert e.value.code == flux._lib.E_INVALID


# ---- flux_host::render_aov_chain ------------------------------------------------------------------------------------------------

def test_cpp_render_aov_chain_refuses_wrong_buffers(tmp_path):
    """It is about host code, so the program is shown no device: the call in order ends in FLUX_E_DEVICE everywhere."""
    exe = selftest.build(str(tmp_path / "aov_chain_host_selftest"), "aov_chain_host_selftest.cpp", host=True, compiler="g++")
    assert "all ok" in selftest.run(exe, env=switches.clean_env(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))


def test_cpp_render_aov_chain_under_asan_and_ubsan(tmp_path):
    """The same program as a stand-alone sanitized executable: the host layer it calls is compiled into it with
    -fsanitize=address,undefined.  It is about host code, so it is shown no device: the call in order ends in FLUX_E_DEVICE."""
    exe = selftest.build(str(tmp_path / "aov_chain_host_selftest_san"), "aov_chain_host_selftest.cpp", host=True, flags=selftest.SANITIZE,
                         compiler="g++")
    assert "all ok" in selftest.run(exe, env=selftest.sanitize_env(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))


# ---- the command-line tool ------------------------------------------------------------------------------------------------------

def test_flux_help_names_the_flags():
    flux_bin, _ = host_bins()
    out = subprocess.run([flux_bin, "--help"], capture_output=True, text=True)
    text = out.stderr + out.stdout
    assert out.returncode == 0
    for word in ("--aov-chain", "--denoise-guides", ".chain_albedo.ppm", ".chain_normal.ppm", ".chain_depth.ppm", ".chain_coverage.ppm"):
        assert word in text


@pytest.mark.parametrize("args,words", [
    (["--aov-chain", "6"], ("--aov-chain", "at most the tracing depth 5")),
    (["--aov-chain", "3", "--depth", "2"], ("--aov-chain", "at most the tracing depth 2")),
    (["--aov-chain", "-1"], ("invalid value", "--aov-chain")),
    (["--aov-chain", "two"], ("invalid value", "--aov-chain")),
    (["--denoise", "--denoise-guides", "second"], ("invalid value 'second'", "--denoise-guides")),
    (["--denoise-guides", "chain"], ("--denoise-guides", "needs that flag")),
    (["--aov-chain", "0", "--gpus", "0"], ("--aov-chain", "local GPU")),
    (["--aov-chain", "2", "-L", "-n", "127.0.0.1:1"], ("--aov-chain", "local GPU")),
    (["--denoise", "--denoise-guides", "chain", "--gpus", "0"], ("--denoise", "local GPU")),
], ids=["beyond-depth", "beyond-given-depth", "negative", "no-number", "bad-guides", "guides-alone", "no-gpu", "no-local", "guides-no-gpu"])
def test_flux_refuses_with_status_2_before_any_job(tmp_path, args, words):
    flux_bin, _ = host_bins()
    out = subprocess.run([flux_bin, os.path.join(SCENES, "mirror_glass.yml"), *args, "--outdir", str(tmp_path)],
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 2, (out.returncode, out.stderr)
    for w in words:
        assert w in out.stderr, out.stderr
    assert "Rendering" not in out.stdout and "Connecting" not in out.stdout
    assert os.listdir(tmp_path) == []


# ---- quality: a measurement, asserted only where chain guides win by a tenth or more ----------------------------------

MIRROR_16SPP = 0.675  # measured: MSE with chain guides / MSE with first-hit guides over the mirror sphere's pixels at root 4


def test_chain_guides_on_demo2_with_a_mirror_sphere(flux, oracle_mod, demo2):
    """demo2 with its centre sphere Reflective at 64 x 48, seed 7, depth 5, against the oracle at root 40, seed 11 (§5f's and §5g's
    settings): denoise_moments_spec with first-hit guides and with chain guides.  Measured chain / first: root 2 whole frame 1.017,
    mirror pixels 1.363 (chain guides lose: nothing asserted); root 4 whole frame 0.977 (no tenth: nothing asserted), mirror pixels
    0.675 -- asserted below 1 and within 0.675 x 1.1 (§5h's convention: fixed inputs, the margin covers a retune of the sigmas)."""
    import denoise_moments_spec as dms
    import moments_spec
    from conftest import small_scene
    sd = small_scene(demo2, 64, 48)
    sd.shapes[4].material = flux.ReflectiveData(0.5, (1.0, 0.9, 0.9))
    o = oracle_mod.Oracle(sd, flux.JobConfiguration(40, 5, 50), seed=11)
    try:
        ref = o.render_frame(threads=4)
    finally:
        o.close()

    def mse(x, mask=None):
        d = (x - ref) ** 2
        return float(d.mean() if mask is None else d[mask].mean())
    ratios = {}
    for root in (2, 4):
        spec = path_spec.PathSpec(sd, root, cs.DEPTH, cs.SEED)
        try:
            spec.frame()
            mom = moments_spec.from_samples(spec.sample_radiance)
            first, chain = path_spec.aov_buffers(spec), cs.chain_buffers(spec, 0).buffers
            mirror = (spec.first_hits()[0] == 4).any(axis=2)
        finally:
            spec.close()
        a, b = dms.denoise_moments(mom, first), dms.denoise_moments(mom, chain)
        ratios[root] = (mse(b) / mse(a), mse(b, mirror) / mse(a, mirror))
        print(f"root {root}: chain / first MSE whole frame {ratios[root][0]:.3f}, over the {int(mirror.sum())} mirror pixels {ratios[root][1]:.3f}")
    assert ratios[4][1] < 1.0 and ratios[4][1] <= MIRROR_16SPP * 1.1
