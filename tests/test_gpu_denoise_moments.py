"""The measured-variance denoiser on the GPU (flux_denoise_moments*, flux_amd/csrc/denoise.hip) against its
specification in numpy (tests/denoise_moments_spec.py): parity on synthetic inputs at every size and level count at which the
kernels take another path, determinism, the device-resident call, the renderer's end-to-end call with its quality bounds, and the
command-line tool.

Tolerance (tests/denoise_checks.py, with the helpers both denoiser suites share): |gpu - spec| <= 1e-10 on usable pixels, unusable
pixels bit for bit -- the bound of tests/test_gpu_denoise.py, for its reason."""
import os

import numpy as np
import pytest

import denoise_checks
import denoise_moments_spec as dms
import denoise_spec
import switches
from conftest import SCENES, small_scene
from denoise_checks import MEASURED, SIZES, TOL
from extension_checks import cli_frame, host_bins, small_yaml

pytestmark = pytest.mark.gpu

inputs, spec, assert_matches = MEASURED.inputs, MEASURED.spec, MEASURED.assert_matches


# ---- 1. parity with the spec --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("levels", [1, 5, 8])
@pytest.mark.parametrize("w,h", SIZES)
def test_parity_with_the_spec(flux, w, h, levels):
    """Odd and even level counts: the frame the last level copies unusable pixels from sits in the other plane set each time."""
    mom, aov = inputs(w, h)
    if w >= 8 and h >= 8:  # the four unusable pixels of denoise_spec.synthetic, and a NaN, a negative and an inf variance
        v = mom[..., 3]
        assert (~dms.usable_moments(mom[..., 0:3], v, aov)).sum() == 7 and np.isnan(v).sum() == 1 and (v < 0).sum() == 1
        assert np.isinf(v).sum() == 1 and (v == 0.0).sum() == 2
    got = flux.denoise_moments(mom, aov, levels=levels)
    assert_matches(got, spec(w, h, levels=levels), mom, aov, f"{w}x{h} levels {levels}")


def test_parity_with_other_sigmas_and_an_even_level_count(flux):
    params = dict(levels=4, sigma_l=0.7, sigma_n=1.5, sigma_z=0.02, sigma_a=0.6)
    mom, aov = inputs(70, 45)
    got = flux.denoise_moments(mom, aov, **params)
    assert_matches(got, spec(70, 45, **params), mom, aov, f"70x45 {params}")
    assert not np.array_equal(got, flux.denoise_moments(mom, aov, levels=4), equal_nan=True)  # the parameters arrive


# (70, 45, 4): an even count, so the last level reads the other plane set; (3, 2, 1): the last level is also the first
@pytest.mark.parametrize("w,h,levels", [(70, 45, 5), (70, 45, 4), (16, 12, 8), (1, 40, 3), (3, 2, 1)])
def test_lds_tiles_give_the_bits_of_the_gathers(flux, monkeypatch, w, h, levels):
    """Where the image has room these inputs hold the 7 unusable pixels of dms.synthetic, so both level kernels copy pixels from a
    buffer of 8 doubles per pixel."""
    denoise_checks.lds_tiles_give_the_bits_of_the_gathers(MEASURED, flux, monkeypatch, w, h, levels)


@pytest.mark.parametrize("levels", [1, 2])
def test_unusable_pixels_come_back_as_channels_0_to_2_bit_for_bit(flux, monkeypatch, levels):
    """Channels 4..7 of the unusable pixels hold values found nowhere else: a copy with another stride than 8 or another channel
    offset than 0 brings one of them, or another pixel's colour, into the output.  Through the gathers and through LDS."""
    mom, aov = (np.array(a) for a in inputs(16, 12))
    ok = dms.usable_moments(mom[..., 0:3], mom[..., 3], aov)
    assert (~ok).sum() == 7
    marks = -1000.0 - np.arange(7 * 4, dtype=np.float64).reshape(7, 4)
    mom[~ok, 4:8] = marks
    for lds in ("0", "8"):
        switches.set_switches(monkeypatch, FLUX_DENOISE_LDS_LEVELS=lds)
        got = flux.denoise_moments(mom, aov, levels=levels)
        assert got[~ok].tobytes() == mom[~ok, 0:3].tobytes()
        assert not np.isin(got, marks).any()
    assert_matches(got, spec(16, 12, levels=levels), mom, aov, f"16x12 levels {levels}, marked channels 4..7")


def test_the_variance_channel_is_what_guides_the_filter(flux):
    """The same frame with another v gives another result, and flux_denoise on channels 0..2 yet another: the measured path reads
    channel 3 and not the neighbourhood's luminance.  flux_denoise itself keeps the bits of its own specification."""
    mom, aov = inputs(70, 45)
    got = flux.denoise_moments(mom, aov)
    louder = np.array(mom)
    louder[..., 3] = np.where(np.isfinite(mom[..., 3]) & (mom[..., 3] >= 0), mom[..., 3] * 100.0, mom[..., 3])
    assert not np.array_equal(flux.denoise_moments(louder, aov), got, equal_nan=True)
    rgb = np.ascontiguousarray(mom[..., 0:3])
    spatial = flux.denoise(rgb, aov)
    assert not np.array_equal(spatial, got, equal_nan=True)
    ok = denoise_spec.usable(rgb, aov)
    assert float(np.max(np.abs(spatial[ok] - denoise_spec.denoise(rgb, aov)[ok]))) <= TOL


# ---- 2. determinism and the device-resident call ----------------------------------------------------------------------------------

def test_two_runs_are_bit_equal(flux):
    mom, aov = inputs(70, 45)
    assert flux.denoise_moments(mom, aov).tobytes() == flux.denoise_moments(mom, aov).tobytes()


@pytest.mark.parametrize("levels", [5, 2])
def test_device_call_on_a_stream_equals_the_host_call_and_leaves_its_inputs(flux, levels):
    denoise_checks.device_call_on_a_stream_equals_the_host_call_and_leaves_its_inputs(MEASURED, flux, levels=levels)


# ---- 3. end to end ----------------------------------------------------------------------------------------------------------------

def test_render_denoised_measured_end_to_end(flux, demo1):
    """demo1 at 64 x 48, sample root 4, seed 7 against a render at root 40, seed 11: the frame on which the spatial estimate loses
    (ratio 1.172 on the CPU, tests/test_moments.py; the measured variance 0.568)."""
    sd = small_scene(demo1, 64, 48)
    with flux.Renderer(sd, flux.JobConfiguration(40, 5, 50), seed=11) as r:
        ref = r.render_frame()
    with flux.Renderer(sd, flux.JobConfiguration(4, 5, 50), seed=7) as r:
        mom, aov = r.render_moments(), r.render_aov()
        frame = r.render_frame()
        r.enable_stats(True)
        r.stats(reset=True)
        got = r.render_denoised(variance="measured")
        assert r.stats()["samples"] == 0  # one moments pass, no render beside it: the render kernels' statistics stay empty
        spatial = r.render_denoised()
        assert np.array_equal(spatial, r.render_denoised(variance="spatial"))
        assert np.array_equal(spatial, flux.denoise(frame, aov))  # the default is today's result
        other = r.render_denoised(variance="measured", levels=2, sigma_l=1.0)
        with pytest.raises(flux.FluxError, match="variance") as e:
            r.render_denoised(variance="temporal")
        assert e.value.code == flux._lib.E_INVALID
    assert np.abs(mom[..., 0:3] - frame).max() <= 1e-12
    want = dms.denoise_moments(mom, aov)
    err = float(np.max(np.abs(got - want)))
    base = denoise_spec.mse(frame, ref)
    ratio, ratio_spatial = denoise_spec.mse(got, ref) / base, denoise_spec.mse(spatial, ref) / base
    print(f"denoise_moments end to end: max |render_denoised(measured) - spec| = {err:.2e}; MSE noisy {base:.3e}, ratio measured "
          f"{ratio:.3f}, spatial {ratio_spatial:.3f}")
    assert np.isfinite(got).all() and err <= 1e-9
    assert ratio < 0.8 and ratio < ratio_spatial
    assert float(np.max(np.abs(other - dms.denoise_moments(mom, aov, levels=2, sigma_l=1.0)))) <= 1e-9


# ---- 4. the command-line tool -------------------------------------------------------------------------------------------------------

def test_cli_writes_the_denoised_frame_from_the_measured_variance(flux, tmp_path):
    flux_bin, _ = host_bins()
    scene = small_yaml(os.path.join(SCENES, "demo2.yml"), tmp_path, 64, 48)
    sd = flux.load_scene(scene)
    with flux.Renderer(sd, flux.JobConfiguration(2, 5, 50), seed=7) as r:
        measured = r.render_denoised(variance="measured")
        spatial = r.render_denoised()
    flux.write_ppm(str(tmp_path / "want.ppm"), measured)
    flux.write_ppm(str(tmp_path / "spatial.ppm"), spatial)
    want = open(tmp_path / "want.ppm", "rb").read()
    assert want != open(tmp_path / "spatial.ppm", "rb").read()
    cli_frame(flux_bin, scene, ["-r", "2", "--seed", "7", "--denoise", "--denoise-variance", "measured"], tmp_path / "out")
    assert sorted(os.listdir(tmp_path / "out")) == sorted([sd.scene_name + ".ppm", sd.scene_name + ".denoised.ppm"])
    assert open(tmp_path / "out" / (sd.scene_name + ".denoised.ppm"), "rb").read() == want
    cli_frame(flux_bin, scene, ["-r", "2", "--seed", "7", "--denoise", "--denoise-variance", "spatial"], tmp_path / "spatial")
    assert open(tmp_path / "spatial" / (sd.scene_name + ".denoised.ppm"), "rb").read() == open(tmp_path / "spatial.ppm", "rb").read()
