"""What tests/test_gpu_denoise.py and tests/test_gpu_denoise_moments.py share: the two paths of the a-trous denoiser -- SPATIAL
(flux_denoise over a frame) and MEASURED (flux_denoise_moments over a moments buffer) -- each with its synthetic inputs and its
specification's frames, computed once and shared read-only, the comparison of a GPU frame with the specification, and the bodies
of the tests that both suites run.  Each suite states its own cases and assertions beyond these.

Tolerance: |gpu - spec| <= 1e-10 on usable pixels, unusable pixels bit for bit.  The kernels repeat the specification's operations
in its order (no contraction, IEEE division and sqrt); the one difference is fexp2 (flux_math.h) against np.exp2, at most 2 ulp: about
25 taps x 8 levels x a few ulp ~ 1e-13 on values <= 1.2.  A dropped or misplaced tap moves a pixel by at least 1/256 of a colour
difference.  Measured: DESIGN.md §5f."""
import numpy as np
import pytest

import denoise_moments_spec as dms
import denoise_spec
import switches

TOL = 1e-10
# (W, H): one tile; not a tile multiple, several tiles both ways, level-4 taps at +-32 inside the image; one pixel; one column (five
# tiles high); smaller than a filter
SIZES = [(16, 12), (70, 45), (1, 1), (1, 40), (3, 2)]


class Path:
    """One variance path: `name` is flux_amd's function (and, with _device, its device-resident form)."""

    def __init__(self, name, synthetic, specification, rgb_and_usable):
        self.name, self.synthetic, self.specification, self.rgb_and_usable = name, synthetic, specification, rgb_and_usable
        self._inputs, self._specs = {}, {}

    def inputs(self, w, h):
        if (w, h) not in self._inputs:
            x, aov = self.synthetic(h, w)
            x.setflags(write=False)
            aov.setflags(write=False)
            self._inputs[(w, h)] = (x, aov)
        return self._inputs[(w, h)]

    def spec(self, w, h, **params):
        """The specification's frame for the synthetic input of this size, computed once per parameter set and shared, read-only."""
        key = (w, h, tuple(sorted(params.items())))
        if key not in self._specs:
            self._specs[key] = self.specification(*self.inputs(w, h), **params)
            self._specs[key].setflags(write=False)
        return self._specs[key]

    def run(self, flux, x, aov, **params):
        return getattr(flux, self.name)(x, aov, **params)

    def assert_matches(self, got, want, x, aov, label):
        rgb, ok = self.rgb_and_usable(x, aov)
        assert got.shape == rgb.shape
        assert got[~ok].tobytes() == rgb[~ok].tobytes(), f"{label}: an unusable pixel was not copied bit for bit"
        assert np.isfinite(got[ok]).all(), label
        err = float(np.max(np.abs(got[ok] - want[ok]))) if ok.any() else 0.0
        print(f"{self.name} {label}: max |gpu - spec| = {err:.2e} over {int(ok.sum())} usable pixels, {int((~ok).sum())} unusable")
        assert err <= TOL, (label, err)


SPATIAL = Path("denoise", denoise_spec.synthetic, denoise_spec.denoise, lambda rgb, aov: (rgb, denoise_spec.usable(rgb, aov)))
MEASURED = Path("denoise_moments", dms.synthetic, dms.denoise_moments,
                lambda mom, aov: (mom[..., 0:3], dms.usable_moments(mom[..., 0:3], mom[..., 3], aov)))


def lds_tiles_give_the_bits_of_the_gathers(path, flux, monkeypatch, w, h, levels):
    """The level kernel exists twice (global gathers; one residue class of the step's lattice per block through LDS, chosen per
    level by FLUX_DENOISE_LDS_LEVELS for the measurement of DESIGN.md §5f): the same taps in the same order."""
    x, aov = path.inputs(w, h)
    switches.set_switches(monkeypatch, FLUX_DENOISE_LDS_LEVELS=0)
    gathers = path.run(flux, x, aov, levels=levels)
    switches.set_switches(monkeypatch, FLUX_DENOISE_LDS_LEVELS=8)
    tiles = path.run(flux, x, aov, levels=levels)
    switches.set_switches(monkeypatch, FLUX_DENOISE_LDS_LEVELS=2)
    mixed = path.run(flux, x, aov, levels=levels)
    assert gathers.tobytes() == tiles.tobytes() == mixed.tobytes()
    path.assert_matches(tiles, path.spec(w, h, levels=levels), x, aov, f"{w}x{h} levels {levels} through LDS")


def device_call_on_a_stream_equals_the_host_call_and_leaves_its_inputs(path, flux, **params):
    import torch
    w, h = 70, 45
    x, aov = path.inputs(w, h)
    want = path.run(flux, x, aov, **params)
    call = getattr(flux, path.name + "_device")
    dev = torch.device("cuda", 0)
    need = flux.denoise_work_doubles(w, h)
    d_x, d_aov = torch.from_numpy(x.copy()).to(dev), torch.from_numpy(aov.copy()).to(dev)
    d_out = torch.full((h, w, 3), -7.0, dtype=torch.float64, device=dev)
    d_work = torch.full((need + 16,), -3.0, dtype=torch.float64, device=dev)  # exactly `need` is handed over; a guard band behind it
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        call(w, h, d_x.data_ptr(), d_aov.data_ptr(), d_out.data_ptr(), d_work.data_ptr(), need, stream=stream.cuda_stream, **params)
    stream.synchronize()
    assert d_out.cpu().numpy().tobytes() == want.tobytes()
    assert d_x.cpu().numpy().tobytes() == x.tobytes() and d_aov.cpu().numpy().tobytes() == aov.tobytes()
    assert bool((d_work[need:] == -3.0).all())  # nothing is written past work_doubles
    with pytest.raises(flux.FluxError):
        call(w, h, d_x.data_ptr(), d_aov.data_ptr(), d_out.data_ptr(), d_work.data_ptr(), need - 1)
