"""The first-hit feature buffers without a GPU: the constants of include/flux_abi.h against the Python binding, the argument
checks of the two entry points, the C++ image mapping (flux_host.hpp aov_image) against numpy, the `flux --aov` flag, and the
specification itself (tests/aov_spec.py) on the `open` scene.  The kernel: tests/test_gpu_aov.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import aov_spec
from conftest import ROOT, SCENES
import selftest
from extension_checks import host_bins

KINDS = ("albedo", "normal", "depth", "coverage")


def test_header_constants_are_the_bindings(flux):
    hdr = open(os.path.join(ROOT, "include", "flux_abi.h")).read()
    c = {name: int(v) for name, v in re.findall(r"#define FLUX_AOV_(\w+) (\d+)", hdr)}
    assert c == {"CHANNELS": 8, "ALBEDO": 0, "NORMAL": 3, "DEPTH": 6, "COVERAGE": 7}
    L = flux._lib
    assert (L.AOV_CHANNELS, L.AOV_ALBEDO_OFFSET, L.AOV_NORMAL_OFFSET, L.AOV_DEPTH, L.AOV_COVERAGE) == (8, 0, 3, 6, 7)
    assert flux.AOV_ALBEDO == slice(0, 3) and flux.AOV_NORMAL == slice(3, 6)
    assert (flux.AOV_DEPTH, flux.AOV_COVERAGE, flux.AOV_CHANNELS) == (6, 7, 8)
    for name in ("AOV_ALBEDO", "AOV_NORMAL", "AOV_DEPTH", "AOV_COVERAGE", "AOV_CHANNELS"):
        assert name in flux.__all__
    assert (aov_spec.ALBEDO, aov_spec.NORMAL, aov_spec.DEPTH, aov_spec.COVERAGE, aov_spec.CHANNELS) == \
        (flux.AOV_ALBEDO, flux.AOV_NORMAL, flux.AOV_DEPTH, flux.AOV_COVERAGE, flux.AOV_CHANNELS)
    assert int(re.search(r"#define FLUX_ABI_VERSION (\d+)", hdr).group(1)) == 3  # no version bump: the symbol is the probe
    assert hasattr(flux.Renderer, "render_aov") and hasattr(flux.Renderer, "render_aov_device")


def test_entry_points_check_their_arguments_without_a_device(flux):
    lib = flux._lib.lib
    assert lib.flux_render_aov_rows(None, 0, 0, None) == flux._lib.E_INVALID
    assert "null" in flux._lib.last_error()
    assert lib.flux_render_aov_rows_device(None, 0, 1, 1, None, None) == flux._lib.E_INVALID
    assert "null" in flux._lib.last_error()


# ---- flux_host::aov_image -----------------------------------------------------------------------------------------------------

def _parse(stdout):
    lines = {ln.split()[0]: ln.split()[1:] for ln in stdout.splitlines() if ln.strip()}
    w, h = (int(x) for x in lines["size"])
    aov = np.array([float(x) for x in lines["aov"]]).reshape(h, w, aov_spec.CHANNELS)
    images = {k: np.array([float(x) for x in lines[k]]).reshape(h, w, 3) for k in KINDS}
    return aov, images, [float(x) for x in lines["flat"]]


def test_cpp_image_mapping_equals_numpy(tmp_path):
    exe = selftest.build(str(tmp_path / "aov_host_selftest"), "aov_host_selftest.cpp", host=True, compiler="g++")
    out = selftest.run(exe)
    assert "all ok" in out
    aov, images, flat = _parse(out)
    # the buffer holds the singled-out cases
    assert np.isinf(aov[..., aov_spec.DEPTH]).any() and (aov[..., aov_spec.ALBEDO] > 1.0).any()
    assert (np.abs(aov[..., aov_spec.NORMAL]).sum(axis=2) == 0.0).any()
    for kind in KINDS:
        want = aov_spec.aov_image(aov, kind)
        assert want.shape == images[kind].shape
        assert np.max(np.abs(images[kind] - want)) <= 1e-15, kind
    assert np.all(images["normal"][0, 2] == 0.5)                      # the zero normal
    assert np.all(images["depth"][1, 0] == 0.0)                       # inf depth
    assert np.all(images["depth"][1, 1] == 0.0)                       # the farthest finite depth is t_max
    assert images["albedo"].max() == 1.0 and np.all(images["albedo"][0, 1] == 1.0)
    assert np.allclose(images["normal"][1, 2], 0.5 + 0.5 * np.array([3.0, 4.0, 12.0]) / 13.0, rtol=0, atol=1e-15)
    assert flat == [0.0, 0.0, 0.0]


def test_cpp_image_mapping_under_asan_and_ubsan(tmp_path):
    """The same program as a stand-alone sanitized executable: the host layer it calls is compiled into it with
    -fsanitize=address,undefined."""
    exe = selftest.build(str(tmp_path / "aov_host_selftest_san"), "aov_host_selftest.cpp", host=True, flags=selftest.SANITIZE,
                         compiler="g++")
    assert "all ok" in selftest.run(exe, env=selftest.sanitize_env())


# ---- the command-line tool ------------------------------------------------------------------------------------------------------

def test_flux_help_names_the_flag():
    flux_bin, _ = host_bins()
    out = subprocess.run([flux_bin, "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    assert "--aov" in out.stderr + out.stdout
    for suffix in (".albedo.ppm", ".normal.ppm", ".depth.ppm", ".coverage.ppm"):
        assert suffix in out.stderr + out.stdout


def test_flux_aov_without_a_local_gpu_is_refused_before_any_job(tmp_path):
    flux_bin, _ = host_bins()
    for args in (["--gpus", "0"], ["-L", "-n", "127.0.0.1:1"]):
        out = subprocess.run([flux_bin, os.path.join(SCENES, "demo2.yml"), "--aov", *args, "--outdir", str(tmp_path)],
                             capture_output=True, text=True, timeout=60)
        assert out.returncode != 0
        assert "--aov" in out.stderr and "local GPU" in out.stderr, out.stderr
        assert "Rendering" not in out.stdout and "Connecting" not in out.stdout
    assert os.listdir(tmp_path) == []


# ---- the specification itself ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def open8(flux, oracle_mod):
    return aov_spec.reference(oracle_mod, aov_spec.open_scene(flux), 8)


def test_spec_counts_on_open(open8):
    """The restatement's counts for `open` at sample_root 8: a reference that ignored misses, or built other rays, would not
    reproduce them."""
    aov, facts = open8
    assert facts == {"misses": 1245, "samples": 12288, "partly_covered": 17}
    cov = aov[..., aov_spec.COVERAGE]
    assert np.isclose(cov.sum() * 64, 12288 - 1245, rtol=0, atol=1e-9)
    assert np.count_nonzero((cov > 0) & (cov < 1)) == 17


def test_spec_values_on_open(open8, flux):
    aov, _ = open8
    assert aov.shape == (aov_spec.H, aov_spec.W, 8)
    cov = aov[..., aov_spec.COVERAGE]
    bg = np.array([0.1, 0.2, 0.3])
    empty = cov == 0
    assert empty.any()
    assert np.allclose(aov[empty][:, aov_spec.ALBEDO], bg, rtol=0, atol=1e-15)       # nothing but background
    assert np.all(aov[empty][:, aov_spec.NORMAL] == 0) and np.all(aov[empty][:, aov_spec.DEPTH] == 0)
    full = cov == 1
    nlen = np.linalg.norm(aov[full][:, aov_spec.NORMAL], axis=1)
    assert np.all(nlen <= 1 + 1e-12) and nlen.max() > 0.99                          # a mean of unit vectors
    assert np.all(aov[~empty][:, aov_spec.DEPTH] > 0)
    # the Emissive sphere is unclamped: power 3 * colour
    assert aov[..., aov_spec.ALBEDO].max() > 1.0 and aov[..., aov_spec.ALBEDO].max() <= 3.0 + 1e-12
