"""The a-trous denoiser without a GPU: the properties of its specification (tests/denoise_spec.py), the quality table of DESIGN.md
section 5f reproduced from the oracle's renders, the argument checks of the three entry points (they run before any device call),
the Python names and the `flux --denoise` flag.  The kernels: tests/test_gpu_denoise.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aov_spec
import denoise_spec
from conftest import SCENES, small_scene
import selftest
from extension_checks import host_bins

H, W = 12, 16


def flat_guides(h=H, w=W):
    aov = np.zeros((h, w, 8))
    aov[..., 0:3] = 0.5
    aov[..., 3:6] = (0.0, 1.0, 0.0)
    aov[..., 6] = 5.0
    aov[..., 7] = 1.0
    return aov


def edge_guides():
    aov = flat_guides()
    aov[:, W // 2:, 3:6] = (1.0, 0.0, 0.0)  # a normal edge ...
    aov[:, W // 2:, 6] = 9.0                # ... and a depth edge between the two regions
    return aov


# ---- properties of the specification ----------------------------------------------------------------------------------------------

def test_constant_image_comes_back_exactly():
    const = np.full((H, W, 3), 0.25)
    for aov in (flat_guides(), edge_guides()):
        assert np.array_equal(denoise_spec.denoise(const, aov), const)
    bright = np.full((H, W, 3), (2.0, 1.0, 0.5))  # max_to_one is part of the output
    assert np.array_equal(denoise_spec.denoise(bright, flat_guides()), denoise_spec.max_to_one(bright))


def test_nothing_leaks_across_a_guide_edge():
    step = np.where(np.arange(W)[None, :, None] < W // 2, 0.2, 0.8) * np.ones((H, W, 3))
    out = denoise_spec.denoise(step, edge_guides())
    leak = float(np.abs(out - step).max())
    print(f"denoise spec: largest change of a two-region step image across its normal + depth edge: {leak:.2e}")
    assert leak <= 1e-15
    # without the edge in the guides the same image IS blurred: the bound above is the guides' doing
    assert np.abs(denoise_spec.denoise(step + 0.05 * np.random.default_rng(1).random((H, W, 3)), flat_guides()) - step).max() > 1e-3


def test_unusable_pixels_come_back_bit_for_bit_and_nothing_else_is_touched_by_them():
    rng = np.random.default_rng(3)
    rgb = rng.random((H, W, 3))
    aov = edge_guides()
    rgb[5, 5] = np.nan
    rgb[6, 12, 1] = np.inf
    aov[2, 9, 4] = np.nan   # a NaN normal
    aov[8, 3, 6] = np.nan   # a NaN depth
    out = denoise_spec.denoise(rgb, aov)
    bad = np.zeros((H, W), bool)
    for y, x in ((5, 5), (6, 12), (2, 9), (8, 3)):
        bad[y, x] = True
    assert np.array_equal(denoise_spec.usable(rgb, aov), ~bad)
    assert out[bad].tobytes() == rgb[bad].tobytes()
    assert np.isfinite(out[~bad]).all()
    # an unusable pixel contributes to no other pixel: whatever it holds, the rest of the output keeps its bits
    rgb2, aov2 = rgb.copy(), aov.copy()
    rgb2[5, 5] = (np.inf, -np.inf, 7.0)
    rgb2[6, 12] = (np.nan, 1e300, 0.0)
    aov2[2, 9, 0:3] = 123.0
    aov2[8, 3, 3:6] = -55.0
    assert np.array_equal(denoise_spec.denoise(rgb2, aov2)[~bad], out[~bad])


def test_a_row_of_infinite_depth_gives_no_nan():
    rng = np.random.default_rng(4)
    rgb = rng.random((H, W, 3))
    aov = flat_guides()
    aov[0, :, 6] = np.inf
    out = denoise_spec.denoise(rgb, aov)
    assert np.isfinite(out).all()
    # the infinite row and the finite rows do not mix: filtering the row alone gives the same row
    alone = denoise_spec.denoise(rgb[0:1], aov[0:1])
    assert np.array_equal(out[0:1], alone)


def test_a_black_albedo_pixel_does_not_disturb_a_constant_image():
    const = np.full((H, W, 3), 0.25)
    aov = flat_guides()
    aov[3, 3, 0:3] = 0.0
    assert np.array_equal(denoise_spec.denoise(const, aov), const)


def test_levels_and_defaults():
    rgb, aov = denoise_spec.synthetic(H, W)
    assert np.array_equal(denoise_spec.denoise(rgb, aov), denoise_spec.denoise(rgb, aov, **denoise_spec.DEFAULTS), equal_nan=True)
    one, five = denoise_spec.denoise(rgb, aov, levels=1), denoise_spec.denoise(rgb, aov, levels=5)
    assert not np.array_equal(one, five, equal_nan=True)


# ---- the quality table of DESIGN.md section 5f ----------------------------------------------------------------------------------------

_cfg = lambda flux, root: flux.JobConfiguration(root, 5, 50)  # noqa: E731


@pytest.mark.parametrize("name,root,expected", [("demo2", 2, 0.171), ("demo1", 1, 0.259)])
def test_quality_against_a_converged_render(flux, oracle_mod, name, root, expected):
    """64 x 48, the noisy frame and its feature buffers at seed 7, the reference at sample root 40, seed 11: the filter must at
    least halve the mean squared error (the identity filter scores 1.0; measured on the CPU: 0.171 and 0.259)."""
    sd = small_scene(flux.load_scene(os.path.join(SCENES, name + ".yml")), 64, 48)
    threads = min(16, os.cpu_count() or 1)
    ref = oracle_mod.Oracle(sd, _cfg(flux, 40), seed=11).render_frame(threads=threads)
    noisy = oracle_mod.Oracle(sd, _cfg(flux, root), seed=aov_spec.SEED).render_frame(threads=threads)
    aov, _ = aov_spec.reference(oracle_mod, sd, root)
    den = denoise_spec.denoise(noisy, aov)
    assert np.isfinite(den).all()
    ratio = denoise_spec.mse(den, ref) / denoise_spec.mse(noisy, ref)
    print(f"denoise quality {name} root {root}: MSE noisy {denoise_spec.mse(noisy, ref):.3e}, denoised {denoise_spec.mse(den, ref):.3e}, "
          f"ratio {ratio:.3f} (expected about {expected})")
    assert ratio < 0.5


# ---- the entry points' argument checks: before any device call ------------------------------------------------------------------------

def _params(*v):
    return (C.c_double * 8)(*(list(v) + [0.0] * (8 - len(v))))


def test_flux_denoise_refuses_bad_arguments_without_a_device(flux):
    L = flux._lib
    lib = L.lib
    dp = C.POINTER(C.c_double)
    rgb = np.zeros((2, 3, 3))
    aov = np.zeros((2, 3, 8))
    out = np.zeros((2, 3, 3))
    p = lambda a: a.ctypes.data_as(dp)  # noqa: E731
    ok = _params(5, 2.0, 0.35, 0.1, 0.1)

    def refused(*args, word=None):
        assert lib.flux_denoise(*args) == L.E_INVALID, args
        if word:
            assert word in L.last_error(), L.last_error()

    refused(0, 3, 2, None, p(aov), ok, p(out), word="null")
    refused(0, 3, 2, p(rgb), None, ok, p(out), word="null")
    refused(0, 3, 2, p(rgb), p(aov), ok, None, word="null")
    refused(0, 0, 2, p(rgb), p(aov), ok, p(out), word="width")
    refused(0, 3, 0, p(rgb), p(aov), ok, p(out), word="height")
    refused(0, 1 << 13, (1 << 13) + 1, p(rgb), p(aov), ok, p(out), word="2^26")
    refused(0, 1 << 40, 1 << 40, p(rgb), p(aov), ok, p(out), word="2^26")  # (the product overflows 64 bits)
    for levels in (0.0, 9.0, 2.5, -1.0, float("nan"), float("inf")):
        refused(0, 3, 2, p(rgb), p(aov), _params(levels, 2.0, 0.35, 0.1, 0.1), p(out), word="levels")
    for k, name in ((1, "sigma_l"), (2, "sigma_n"), (3, "sigma_z"), (4, "sigma_a")):
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            v = [5, 2.0, 0.35, 0.1, 0.1]
            v[k] = bad
            refused(0, 3, 2, p(rgb), p(aov), _params(*v), p(out), word=name)
    for k in (5, 6, 7):
        v = [5, 2.0, 0.35, 0.1, 0.1, 0.0, 0.0, 0.0]
        v[k] = 1.0
        refused(0, 3, 2, p(rgb), p(aov), _params(*v), p(out), word="reserved")
    # valid arguments get past the checks: whatever comes back then is about the device, not the arguments
    rc = lib.flux_denoise(0, 3, 2, p(rgb), p(aov), None, p(out))
    assert rc in (L.FLUX_OK, L.E_DEVICE), (rc, L.last_error())


def test_flux_denoise_device_refuses_bad_arguments_without_a_device(flux):
    L = flux._lib
    lib = L.lib
    w, h = 5, 4
    need = lib.flux_denoise_work_doubles(w, h)
    assert need >= w * h * 11  # colour, albedo, normal, depth and variance of every pixel at least
    assert lib.flux_denoise_work_doubles(0, 4) == 0 and lib.flux_denoise_work_doubles(4, 0) == 0
    assert lib.flux_denoise_work_doubles(1 << 13, (1 << 13) + 1) == 0 and lib.flux_denoise_work_doubles(1 << 40, 1 << 40) == 0
    assert lib.flux_denoise_work_doubles(1 << 13, 1 << 13) > 0
    assert flux.denoise_work_doubles(w, h) == need
    rgb, aov, out, work = 0x1000, 0x2000, 0x3000, 0x4000  # never dereferenced: the checks refuse first

    def refused(*args, word=None):
        assert lib.flux_denoise_device(*args) == L.E_INVALID, args
        if word:
            assert word in L.last_error(), L.last_error()

    for k in range(4):
        ptrs = [rgb, aov, out, work]
        ptrs[k] = None
        refused(0, w, h, ptrs[0], ptrs[1], None, ptrs[2], ptrs[3], need, None, word="null")
    refused(0, 0, h, rgb, aov, None, out, work, need, None, word="width")
    refused(0, w, 0, rgb, aov, None, out, work, need, None, word="height")
    refused(0, 1 << 13, (1 << 13) + 1, rgb, aov, None, out, work, 1 << 62, None, word="2^26")
    refused(0, w, h, rgb, aov, _params(0, 2.0, 0.35, 0.1, 0.1), out, work, need, None, word="levels")
    refused(0, w, h, rgb, aov, _params(5, 2.0, 0.0, 0.1, 0.1), out, work, need, None, word="sigma_n")
    refused(0, w, h, rgb, aov, _params(5, 2.0, 0.35, 0.1, 0.1, 0.0, 3.0), out, work, need, None, word="reserved")
    refused(0, w, h, rgb, aov, None, out, work, need - 1, None, word="work_doubles")
    refused(0, w, h, rgb, aov, None, out, work, 0, None, word="work_doubles")
    refused(0, w, h, rgb, aov, None, rgb, work, need, None, word="d_out_rgb")
    refused(0, w, h, rgb, aov, None, work, work, need, None, word="d_out_rgb")
    with pytest.raises(flux.FluxError) as e:
        flux.denoise_device(w, h, rgb, aov, out, work, need - 1)
    assert e.value.code == L.E_INVALID


def test_python_names(flux):
    for name in ("denoise", "denoise_device", "denoise_work_doubles"):
        assert name in flux.__all__ and callable(getattr(flux, name))
    assert hasattr(flux.Renderer, "render_denoised")
    for name in ("flux_denoise", "flux_denoise_work_doubles", "flux_denoise_device"):
        assert name in flux._lib.SYMBOLS
    assert flux._lib.DENOISE_PARAM_WORDS == 8
    hdr = open(os.path.join(os.path.dirname(SCENES), "include", "flux_abi.h")).read()
    assert "#define FLUX_DENOISE_PARAM_WORDS 8" in hdr and "#define FLUX_ABI_VERSION 3" in hdr
    with pytest.raises(flux.FluxError) as e:  # shapes that do not belong together never reach the library
        flux.denoise(np.zeros((2, 3, 3)), np.zeros((2, 4, 8)))
    assert e.value.code == flux._lib.E_INVALID
    with pytest.raises(flux.FluxError, match="levels"):
        flux.denoise(np.zeros((2, 3, 3)), np.zeros((2, 3, 8)), levels=9)


# ---- flux_host::denoise_frame ----------------------------------------------------------------------------------------------------------

def test_cpp_denoise_frame_checks_its_buffers(tmp_path):
    exe = selftest.build(str(tmp_path / "denoise_host_selftest"), "denoise_host_selftest.cpp", host=True, compiler="g++")
    out = selftest.run(exe)
    assert "all ok" in out


# ---- the command-line tool --------------------------------------------------------------------------------------------------------------

def test_flux_help_names_the_flag_and_the_file():
    flux_bin, _ = host_bins()
    out = subprocess.run([flux_bin, "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    assert "--denoise" in out.stderr + out.stdout and ".denoised.ppm" in out.stderr + out.stdout


def test_flux_denoise_without_a_local_gpu_is_refused_before_any_job(tmp_path):
    flux_bin, _ = host_bins()
    for args in (["--gpus", "0"], ["-L", "-n", "127.0.0.1:1"], ["--aov", "--gpus", "0"]):
        out = subprocess.run([flux_bin, os.path.join(SCENES, "demo2.yml"), "--denoise", *args, "--outdir", str(tmp_path)],
                             capture_output=True, text=True, timeout=60)
        assert out.returncode == 2, (out.returncode, out.stderr)
        assert "local GPU" in out.stderr and ("--denoise" in out.stderr or "--aov" in args), out.stderr
        assert "Rendering" not in out.stdout and "Connecting" not in out.stdout
    assert os.listdir(tmp_path) == []
