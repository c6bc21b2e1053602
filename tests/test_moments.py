"""The per-pixel sample moments and the measured-variance denoiser without a GPU: the numpy specifications
(tests/moments_spec.py, tests/denoise_moments_spec.py) and their properties, the conditions the GPU suite's scenes must meet, the
quality table recomputed from tests/path_spec.py's samples, the argument checks of the four entry points (they run before any
device call), the Python names, flux_host::denoise_moments_frame and the `flux --denoise-variance` flag.
The kernels: tests/test_gpu_moments.py, tests/test_gpu_denoise_moments.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_moments_spec as dms
import denoise_spec
import moments_spec as ms
from conftest import ROOT, SCENES, small_scene
import selftest
from extension_checks import host_bins
from path_spec import aov_buffers, PathSpec

H, W = 12, 16


# ---- moments_spec -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,root", list(ms.CASES), ids=[f"{n}-{r}" for n, r in ms.CASES])
def test_spec_and_scene_conditions(flux, name, root):
    """Channels 0..2 are PathSpec.frame() bit for bit, the one-pass s2 is numpy's two-pass one to 1e-12 (s2 + m²), and the scene has
    the noisy, zero-variance and clamped pixels the comparison with the kernel relies on, with no decision at rounding level."""
    sd, mom, rad, frame, margin = ms.reference(flux, name, root)
    assert mom.shape == (ms.H, ms.W, 8) and rad.shape == (ms.H, ms.W, root * root, 3)
    assert mom[..., ms.RGB].tobytes() == np.ascontiguousarray(frame).tobytes()
    two_pass, m2 = ms.two_pass_s2(rad), ms.mean_lum(rad) ** 2
    err = float((np.abs(mom[..., ms.S2] - two_pass) - 1e-12 * (two_pass + m2)).max())
    got = ms.counts(mom, rad)
    print(f"moments spec {name} root {root}: noisy / zero-variance / clamped pixels {got}, min margin {margin:.2e}, "
          f"largest |one-pass - two-pass| s2 over its bound: {err:.2e}")
    assert err <= 0.0
    assert got == ms.CASES[(name, root)]
    assert margin >= ms.MIN_MARGIN
    # channel 3 is channel 7 / N where nothing is clamped, and smaller by k² where max_to_one scaled the pixel
    clamped = mom[..., ms.MEAN].max(axis=2) > 1.0
    N = root * root
    assert np.array_equal(mom[..., ms.VAR][~clamped], (mom[..., ms.S2] / N)[~clamped])
    scaled = clamped & (mom[..., ms.S2] > 0.0)
    assert np.all(mom[..., ms.VAR][scaled] < (mom[..., ms.S2] / N)[scaled]) and np.all(mom[..., ms.VAR][clamped & ~scaled] == 0.0)
    assert np.all(mom[..., ms.S2] >= 0.0) and np.isfinite(mom).all()


def test_spec_shows_a_nan_or_inf_sample_in_the_variance_channels():
    rad = np.random.default_rng(5).random((1, 3, 4, 3))
    rad[0, 1, 2, 0] = np.nan
    rad[0, 2, 1, 1] = np.inf
    mom = ms.from_samples(rad)
    assert np.isfinite(mom[0, 0]).all()
    for x in (1, 2):
        assert np.isnan(mom[0, x, ms.VAR]) and np.isnan(mom[0, x, ms.S2])
    const = np.full((1, 1, 9, 3), 0.3)   # all samples equal: exactly 0, never negative
    assert ms.from_samples(const)[0, 0, ms.S2] == 0.0 and ms.from_samples(const)[0, 0, ms.VAR] == 0.0


# ---- denoise_moments_spec ---------------------------------------------------------------------------------------------------------

def flat_guides(h=H, w=W):
    aov = np.zeros((h, w, 8))
    aov[..., 0:3] = 0.5
    aov[..., 3:6] = (0.0, 1.0, 0.0)
    aov[..., 6] = 5.0
    aov[..., 7] = 1.0
    return aov


def as_moments(rgb, v):
    mom = np.zeros(rgb.shape[:2] + (8,))
    mom[..., 0:3], mom[..., 3], mom[..., 4:7], mom[..., 7] = rgb, v, rgb, v
    return mom


def test_constant_image_comes_back_exactly_whatever_the_variance():
    const = np.full((H, W, 3), 0.25)
    rng = np.random.default_rng(2)
    for v in (np.zeros((H, W)), np.full((H, W), 1e-3), rng.random((H, W)) * 10.0, np.full((H, W), 1e300)):
        assert np.array_equal(dms.denoise_moments(as_moments(const, v), flat_guides()), const)
    bright = np.full((H, W, 3), (2.0, 1.0, 0.5))
    assert np.array_equal(dms.denoise_moments(as_moments(bright, rng.random((H, W))), flat_guides()), denoise_spec.max_to_one(bright))


def test_a_pixel_with_an_unusable_variance_comes_back_bit_for_bit_and_touches_nothing_else():
    rng = np.random.default_rng(3)
    rgb = rng.random((H, W, 3))
    v = 0.01 * rng.random((H, W))
    bad = np.zeros((H, W), bool)
    for (y, x), val in (((5, 5), np.nan), ((6, 12), np.inf), ((2, 9), -1e-300), ((8, 3), -np.inf)):
        v[y, x] = val
        bad[y, x] = True
    aov = flat_guides()
    out = dms.denoise_moments(as_moments(rgb, v), aov)
    assert np.array_equal(dms.usable_moments(rgb, v, aov), ~bad)
    assert out[bad].tobytes() == rgb[bad].tobytes()
    assert np.isfinite(out).all()
    rgb2, v2 = rgb.copy(), v.copy()
    rgb2[5, 5], rgb2[6, 12] = (np.inf, -np.inf, 7.0), (1e300, 0.0, np.nan)
    v2[2, 9], v2[8, 3] = np.nan, -5.0
    assert np.array_equal(dms.denoise_moments(as_moments(rgb2, v2), aov)[~bad], out[~bad])
    # a zero is a usable variance
    v3 = v.copy()
    v3[5, 5] = 0.0
    assert dms.usable_moments(rgb, v3, aov)[5, 5]


def test_a_zero_variance_pixel_among_noisy_neighbours_is_filtered():
    """What the prefilter is for: with its own variance of exactly 0 the pixel would refuse every neighbour (sd = 1e-8) and come
    back as it went in; with the neighbourhood's variance it is filtered like them."""
    rng = np.random.default_rng(4)
    rgb = 0.5 + 0.1 * rng.standard_normal((H, W, 3))
    v = np.full((H, W), 0.01)
    v[6, 8] = 0.0
    mom = as_moments(rgb, v)
    out = dms.denoise_moments(mom, flat_guides())
    assert np.abs(out[6, 8] - rgb[6, 8]).max() > 1e-3
    raw = dms.denoise_moments(mom, flat_guides(), prefilter=False)
    assert np.abs(raw[6, 8] - rgb[6, 8]).max() < 1e-6


# ---- the quality table of DESIGN.md section 5g ----------------------------------------------------------------------------------------

QUALITY = [("demo2", 2), ("demo2", 4), ("demo1", 2), ("demo1", 4), ("demo1", 8)]
_quality = {}


def quality(flux, oracle_mod, name, root):
    """MSE ratios denoised / noisy of the three filters for one row of the table: 64 x 48, the noisy frame, its moments and its
    feature buffers from PathSpec at seed 7, the reference from the restatement at sample root 40, seed 11."""
    if (name, root) not in _quality:
        sd = small_scene(flux.load_scene(os.path.join(SCENES, name + ".yml")), 64, 48)
        ref = oracle_mod.Oracle(sd, flux.JobConfiguration(40, 5, 50), seed=11).render_frame(threads=min(16, os.cpu_count() or 1))
        spec = PathSpec(sd, root, 5, 7)
        try:
            noisy = spec.frame()
            mom = ms.from_samples(spec.sample_radiance)
            aov = aov_buffers(spec)
            zero = float(np.count_nonzero(ms.two_pass_s2(spec.sample_radiance) == 0.0)) / (64 * 48)
        finally:
            spec.close()
        assert np.array_equal(mom[..., 0:3], noisy)
        base = denoise_spec.mse(noisy, ref)
        _quality[(name, root)] = (denoise_spec.mse(denoise_spec.denoise(noisy, aov), ref) / base,
                                  denoise_spec.mse(dms.denoise_moments(mom, aov, prefilter=False), ref) / base,
                                  denoise_spec.mse(dms.denoise_moments(mom, aov), ref) / base, zero)
    return _quality[(name, root)]


@pytest.mark.parametrize("name,root", QUALITY, ids=[f"{n}-{r}" for n, r in QUALITY])
def test_quality_against_a_converged_render(flux, oracle_mod, name, root):
    spatial, raw, measured, zero = quality(flux, oracle_mod, name, root)
    print(f"denoise_moments quality {name} root {root}: MSE ratio spatial {spatial:.3f}, measured as-is {raw:.3f}, "
          f"measured prefiltered {measured:.3f}; pixels whose samples are all equal: {100 * zero:.0f} %")
    assert measured < spatial
    if (name, root) == ("demo2", 2):
        assert measured < 0.5
    if (name, root) == ("demo1", 4):
        assert measured < 0.8  # the identity filter scores 1.0, the spatial estimate 1.172


# ---- the entry points' argument checks: before any device call ------------------------------------------------------------------------

def _params(*v):
    return (C.c_double * 8)(*(list(v) + [0.0] * (8 - len(v))))


def test_flux_denoise_moments_refuses_bad_arguments_without_a_device(flux):
    L = flux._lib
    lib = L.lib
    dp = C.POINTER(C.c_double)
    mom, aov, out = np.zeros((2, 3, 8)), np.zeros((2, 3, 8)), np.zeros((2, 3, 3))
    p = lambda a: a.ctypes.data_as(dp)  # noqa: E731
    ok = _params(5, 2.0, 0.35, 0.1, 0.1)

    def refused(*args, word):
        assert lib.flux_denoise_moments(*args) == L.E_INVALID, args
        assert word in L.last_error(), L.last_error()

    refused(0, 3, 2, None, p(aov), ok, p(out), word="null")
    refused(0, 3, 2, p(mom), None, ok, p(out), word="null")
    refused(0, 3, 2, p(mom), p(aov), ok, None, word="null")
    refused(0, 0, 2, p(mom), p(aov), ok, p(out), word="width")
    refused(0, 3, 0, p(mom), p(aov), ok, p(out), word="height")
    refused(0, 1 << 13, (1 << 13) + 1, p(mom), p(aov), ok, p(out), word="2^26")
    refused(0, 1 << 40, 1 << 40, p(mom), p(aov), ok, p(out), word="2^26")
    for levels in (0.0, 9.0, 2.5, float("nan")):
        refused(0, 3, 2, p(mom), p(aov), _params(levels, 2.0, 0.35, 0.1, 0.1), p(out), word="levels")
    for k, name in ((1, "sigma_l"), (2, "sigma_n"), (3, "sigma_z"), (4, "sigma_a")):
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            v = [5, 2.0, 0.35, 0.1, 0.1]
            v[k] = bad
            refused(0, 3, 2, p(mom), p(aov), _params(*v), p(out), word=name)
    refused(0, 3, 2, p(mom), p(aov), _params(5, 2.0, 0.35, 0.1, 0.1, 0.0, 0.0, 1.0), p(out), word="reserved")
    rc = lib.flux_denoise_moments(0, 3, 2, p(mom), p(aov), None, p(out))
    assert rc in (L.FLUX_OK, L.E_DEVICE), (rc, L.last_error())


def test_flux_denoise_moments_device_refuses_bad_arguments_without_a_device(flux):
    L = flux._lib
    lib = L.lib
    w, h = 5, 4
    need = lib.flux_denoise_work_doubles(w, h)
    mom, aov, out, work = 0x1000, 0x2000, 0x3000, 0x4000  # never dereferenced: the checks refuse first

    def refused(*args, word):
        assert lib.flux_denoise_moments_device(*args) == L.E_INVALID, args
        assert word in L.last_error(), L.last_error()

    for k in range(4):
        ptrs = [mom, aov, out, work]
        ptrs[k] = None
        refused(0, w, h, ptrs[0], ptrs[1], None, ptrs[2], ptrs[3], need, None, word="null")
    refused(0, 0, h, mom, aov, None, out, work, need, None, word="width")
    refused(0, w, 0, mom, aov, None, out, work, need, None, word="height")
    refused(0, 1 << 13, (1 << 13) + 1, mom, aov, None, out, work, 1 << 62, None, word="2^26")
    refused(0, w, h, mom, aov, _params(0, 2.0, 0.35, 0.1, 0.1), out, work, need, None, word="levels")
    refused(0, w, h, mom, aov, _params(5, 2.0, 0.0, 0.1, 0.1), out, work, need, None, word="sigma_n")
    refused(0, w, h, mom, aov, _params(5, 2.0, 0.35, 0.1, 0.1, 0.0, 3.0), out, work, need, None, word="reserved")
    refused(0, w, h, mom, aov, None, out, work, need - 1, None, word="work_doubles")
    refused(0, w, h, mom, aov, None, mom, work, need, None, word="d_out_rgb")
    refused(0, w, h, mom, aov, None, work, work, need, None, word="d_out_rgb")
    with pytest.raises(flux.FluxError) as e:
        flux.denoise_moments_device(w, h, mom, aov, out, work, need - 1)
    assert e.value.code == L.E_INVALID


def test_flux_render_moments_refuses_a_null_context_and_null_pointers(flux):
    """The context-free refusals of the two render entry points; the ones that need a context are in tests/test_gpu_moments.py."""
    L = flux._lib
    out = np.zeros(8)
    assert L.lib.flux_render_moments_rows(None, 0, 0, out.ctypes.data_as(C.POINTER(C.c_double))) == L.E_INVALID
    assert "null context" in L.last_error()
    assert L.lib.flux_render_moments_rows_device(None, 0, 1, 1, 0x1000, None) == L.E_INVALID
    assert "null context" in L.last_error()


def test_python_names(flux):
    for name in ("denoise_moments", "denoise_moments_device", "MOMENT_RGB", "MOMENT_VAR", "MOMENT_MEAN", "MOMENT_S2", "MOMENT_CHANNELS"):
        assert name in flux.__all__ and hasattr(flux, name)
    assert (flux.MOMENT_RGB, flux.MOMENT_VAR, flux.MOMENT_MEAN, flux.MOMENT_S2, flux.MOMENT_CHANNELS) == (slice(0, 3), 3, slice(4, 7), 7, 8)
    for name in ("render_moments", "render_moments_device", "render_denoised"):
        assert hasattr(flux.Renderer, name)
    for name in ("flux_render_moments_rows", "flux_render_moments_rows_device", "flux_denoise_moments", "flux_denoise_moments_device"):
        assert name in flux._lib.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "flux_abi.h")).read()
    for line in ("#define FLUX_MOMENT_CHANNELS 8", "#define FLUX_MOMENT_RGB 0", "#define FLUX_MOMENT_VAR 3", "#define FLUX_MOMENT_MEAN 4",
                 "#define FLUX_MOMENT_S2 7", "#define FLUX_ABI_VERSION 3"):
        assert line in hdr, line
    with pytest.raises(flux.FluxError) as e:  # shapes that do not belong together never reach the library
        flux.denoise_moments(np.zeros((2, 3, 3)), np.zeros((2, 3, 8)))
    assert e.value.code == flux._lib.E_INVALID
    with pytest.raises(flux.FluxError, match="levels"):
        flux.denoise_moments(np.zeros((2, 3, 8)), np.zeros((2, 3, 8)), levels=9)


def test_render_denoised_refuses_an_unknown_variance():
    """The check sits in front of every render call, so no context is needed to see it."""
    import flux_amd
    with pytest.raises(flux_amd.FluxError, match="variance") as e:
        flux_amd.Renderer.render_denoised(None, variance="temporal")
    assert e.value.code == flux_amd._lib.E_INVALID


# ---- flux_host::denoise_moments_frame -------------------------------------------------------------------------------------------------

def test_cpp_denoise_moments_frame_checks_its_buffers(tmp_path):
    exe = selftest.build(str(tmp_path / "moments_host_selftest"), "moments_host_selftest.cpp", host=True, compiler="g++")
    out = selftest.run(exe)
    assert "all ok" in out


def test_cpp_denoise_moments_frame_under_sanitizers(tmp_path):
    """The same program as a stand-alone sanitized executable: the host layer it calls is compiled into it with
    -fsanitize=address,undefined.  It is about host code, so it is shown no device: the valid call ends in FLUX_E_DEVICE everywhere."""
    exe = selftest.build(str(tmp_path / "moments_host_selftest_san"), "moments_host_selftest.cpp", host=True, flags=selftest.SANITIZE,
                         compiler="g++")
    assert "all ok" in selftest.run(exe, env=selftest.sanitize_env(HIP_VISIBLE_DEVICES="-1"))


# ---- the command-line tool --------------------------------------------------------------------------------------------------------------

def test_flux_help_names_the_flag():
    flux_bin, _ = host_bins()
    out = subprocess.run([flux_bin, "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    assert "--denoise-variance" in out.stderr + out.stdout and "measured" in out.stderr + out.stdout


def test_flux_denoise_variance_is_refused_without_denoise_or_with_another_word(tmp_path):
    flux_bin, _ = host_bins()
    scene = os.path.join(SCENES, "demo2.yml")
    for args, word in ((["--denoise-variance", "measured"], "--denoise"), (["--denoise", "--denoise-variance", "temporal"], "temporal"),
                       (["--denoise", "--denoise-variance"], "requires a value")):
        out = subprocess.run([flux_bin, scene, "--outdir", str(tmp_path), *args], capture_output=True, text=True, timeout=60)
        assert out.returncode == 2, (args, out.returncode, out.stderr)
        assert "--denoise-variance" in out.stderr and word in out.stderr, out.stderr
        assert "Rendering" not in out.stdout and "Connecting" not in out.stdout
    # with --denoise and a known word the flag is accepted: what refuses the run here is the missing local GPU
    out = subprocess.run([flux_bin, scene, "--denoise", "--denoise-variance", "measured", "--gpus", "0", "--outdir", str(tmp_path)],
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "local GPU" in out.stderr, out.stderr
    assert os.listdir(tmp_path) == []
