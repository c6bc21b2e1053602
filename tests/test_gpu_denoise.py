"""The a-trous denoiser on the GPU (flux_denoise*, flux_amd/csrc/denoise.hip) against its specification in numpy
(tests/denoise_spec.py): parity on synthetic inputs at every size and level count at which the kernels take another path,
determinism, the device-resident call, the renderer's end-to-end call with its quality bound, and the command-line tool.

Tolerance (tests/denoise_checks.py, with the helpers both denoiser suites share): |gpu - spec| <= 1e-10 on usable pixels, unusable
pixels bit for bit."""
import os

import numpy as np
import pytest

import denoise_checks
import denoise_spec
from conftest import SCENES, small_scene
from denoise_checks import SIZES, SPATIAL, TOL
from extension_checks import cli_frame, host_bins, small_yaml

pytestmark = pytest.mark.gpu

inputs, spec, assert_matches = SPATIAL.inputs, SPATIAL.spec, SPATIAL.assert_matches


# ---- 1. parity with the spec --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("levels", [1, 5, 8])
@pytest.mark.parametrize("w,h", SIZES)
def test_parity_with_the_spec(flux, w, h, levels):
    """At 8 levels the last step is 128: every tap but the centre lies off every one of these images."""
    rgb, aov = inputs(w, h)
    if w >= 8 and h >= 8:
        assert (~denoise_spec.usable(rgb, aov)).sum() == 4 and np.isinf(aov[0, :, 6]).all() and (aov[3, 3, 0:3] == 0).all()
    got = flux.denoise(rgb, aov, levels=levels)
    assert_matches(got, spec(w, h, levels=levels), rgb, aov, f"{w}x{h} levels {levels}")


def test_parity_with_other_sigmas(flux):
    params = dict(levels=3, sigma_l=0.7, sigma_n=1.5, sigma_z=0.02, sigma_a=0.6)
    rgb, aov = inputs(70, 45)
    got = flux.denoise(rgb, aov, **params)
    assert_matches(got, spec(70, 45, **params), rgb, aov, f"70x45 {params}")
    assert not np.array_equal(got, flux.denoise(rgb, aov, levels=3), equal_nan=True)  # the parameters arrive


@pytest.mark.parametrize("w,h,levels", [(70, 45, 5), (16, 12, 8), (1, 40, 3)])
def test_lds_tiles_give_the_bits_of_the_gathers(flux, monkeypatch, w, h, levels):
    denoise_checks.lds_tiles_give_the_bits_of_the_gathers(SPATIAL, flux, monkeypatch, w, h, levels)


# ---- 2. determinism and the device-resident call ----------------------------------------------------------------------------------

def test_two_runs_are_bit_equal(flux):
    rgb, aov = inputs(70, 45)
    assert flux.denoise(rgb, aov).tobytes() == flux.denoise(rgb, aov).tobytes()


def test_device_call_on_a_stream_equals_the_host_call_and_leaves_its_inputs(flux):
    denoise_checks.device_call_on_a_stream_equals_the_host_call_and_leaves_its_inputs(SPATIAL, flux)


# ---- 3. end to end ----------------------------------------------------------------------------------------------------------------

def test_render_denoised_end_to_end(flux, demo2):
    """demo2 at 64 x 48, sample root 2, seed 7 against a render at root 40, seed 11 (the GPU's frame equals the oracle's to 1e-4,
    tests/test_gpu_parity.py; on the oracle's frames the ratio is 0.171, tests/test_denoise.py)."""
    sd = small_scene(demo2, 64, 48)
    with flux.Renderer(sd, flux.JobConfiguration(40, 5, 50), seed=11) as r:
        ref = r.render_frame()
    with flux.Renderer(sd, flux.JobConfiguration(2, 5, 50), seed=7) as r:
        r.enable_stats(True)
        r.stats(reset=True)
        frame = r.render_frame()
        stats, plan = r.stats(), r.launch_plan()
        aov = r.render_aov()
        r.stats(reset=True)
        got = r.render_denoised()
        assert r.stats() == stats and r.launch_plan() == plan  # one render_frame's worth, and the same plan
        r.stats(reset=True)
        assert np.array_equal(r.render_frame(), frame) and r.stats() == stats
        other = r.render_denoised(levels=2, sigma_l=1.0)
    want = denoise_spec.denoise(frame, aov)
    err = float(np.max(np.abs(got - want)))
    ratio = denoise_spec.mse(got, ref) / denoise_spec.mse(frame, ref)
    print(f"denoise end to end: max |render_denoised - spec| = {err:.2e}; MSE noisy {denoise_spec.mse(frame, ref):.3e}, denoised "
          f"{denoise_spec.mse(got, ref):.3e}, ratio {ratio:.3f}")
    assert np.isfinite(got).all() and err <= TOL
    assert ratio < 0.5
    assert float(np.max(np.abs(other - denoise_spec.denoise(frame, aov, levels=2, sigma_l=1.0)))) <= TOL


# ---- 4. the command-line tool -------------------------------------------------------------------------------------------------------

def test_cli_writes_the_denoised_frame(flux, tmp_path):
    flux_bin, _ = host_bins()
    scene = small_yaml(os.path.join(SCENES, "demo2.yml"), tmp_path, 64, 48)
    sd = flux.load_scene(scene)
    with flux.Renderer(sd, flux.JobConfiguration(2, 5, 50), seed=7) as r:
        frame, aov = r.render_frame(), r.render_aov()
    flux.write_ppm(str(tmp_path / "want.ppm"), flux.denoise(frame, aov))
    want = open(tmp_path / "want.ppm", "rb").read()
    cli_frame(flux_bin, scene, ["-r", "2", "--seed", "7", "--denoise"], tmp_path / "out")
    assert sorted(os.listdir(tmp_path / "out")) == sorted([sd.scene_name + ".ppm", sd.scene_name + ".denoised.ppm"])
    assert open(tmp_path / "out" / (sd.scene_name + ".denoised.ppm"), "rb").read() == want
    cli_frame(flux_bin, scene, ["-r", "2", "--seed", "7", "--aov", "--denoise"], tmp_path / "both")
    assert sorted(os.listdir(tmp_path / "both")) == sorted([sd.scene_name + ".ppm", sd.scene_name + ".denoised.ppm"] +
                                                           [f"{sd.scene_name}.{k}.ppm" for k in ("albedo", "normal", "depth", "coverage")])
    assert open(tmp_path / "both" / (sd.scene_name + ".denoised.ppm"), "rb").read() == want
