"""The reduced arms of the split kernel's first-plane test divide without the general division's scaffolding (flux_amd/csrc/
flux_plane_axis.h plane_div_unscaled), behind votes that hold d_a to plane_div_admits; and the TYP instantiations read the depth cut's
depth with the depth limit, in one load in front of the scan (RenderParams::depth_pair).

1. The probe (flux_debug_plane_div): the unscaled function and `/`, both on the device, and the votes' word on den, for about 2e5 operand
   pairs -- random admitted pairs, the edges of both operands (a den whose fraction bits are all ones among them: the hard case of the
   sequence's last step, where the CPU test cannot hold a moved seed to `/`; the device's own seed against the device's own `/` must
   agree), and pairs OUTSIDE the predicate, of which only the votes' answer is checked.  Bit equality on every admitted pair whose num
   lies in the range the header states (2^-894 <= |num| < 2^499); for a smaller num -- zeros and denormals -- both forms stay below
   2^-764, the plane is missed either way (tests/test_plane_div.py says why bit equality is not asked there).  The predicate as a
   function of the lane and as the wave mask the kernel's votes take agree with each other and with the host's f32 conversion.

2. Frames of 8 x 6 pixels at sample root 16 (256 spp, the smallest count the split kernel takes) and 23 (a last batch that is not full),
   depth limit 5 and 1, demo2 turned so that the floor's normal is each of +-x, +-y, +-z, with the hit queue and with
   FLUX_SPLIT_HITQ_CAP=0, with FLUX_SPLIT_DEPTH_CUT=0 and =1: bit-equal to FLUX_PLANE_AXIS=0 (general dot products, IEEE `/`), path statistics equal to the oracle's.

3. A camera that looks along the floor, a hair above it: primary rays graze the plane (|d_a| down to 1e-4 and smaller).  Bit-equal to
   FLUX_PLANE_AXIS=0 again.  Which arm a wave took cannot be read from a launch of the product library -- it keeps no counter of it (the
   census is a debug build's) -- and no scene built on the CPU oracle is known to put a |d_a| below 2^-126 into a lane that is not
   exactly zero there; a zero d_a (a horizontal primary ray) is what this camera can produce, and whether a sample does is not
   asserted.  The general arm's side of the vote rests on the probe above."""
import copy

import numpy as np
import pytest

import split_checks as sc
from conftest import small_scene
from split_checks import TURNS
from switches import switches  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu

SEED = 4
JOBS = ((16, 5), (16, 1), (23, 5), (23, 1))  # (sample root, depth limit)
KERNELS = [dict(FLUX_SPLIT_DEPTH_CUT=cut, **queue) for queue in ({}, {"FLUX_SPLIT_HITQ_CAP": "0"}) for cut in ("0", "1")]

NUM_LOW, NUM_HIGH, SMALL = 2.0 ** -894, 2.0 ** 499, 2.0 ** -764
FLT_MIN, FLT_MAX = np.float32(2.0 ** -126), np.finfo(np.float32).max


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _host_admits(den):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        f = np.abs(den.astype(np.float32))
    return (f >= FLT_MIN) & (f <= FLT_MAX)  # (a NaN fails both)


def _pairs():
    rng = np.random.default_rng(11)
    sign = lambda n: rng.choice([-1.0, 1.0], n)  # noqa: E731
    n = 60000
    dens = [rng.uniform(-1.0, 1.0, n),                                                 # a direction's component
            sign(n) * np.ldexp(rng.uniform(0.5, 1.0, n), rng.integers(-125, 129, n)),  # every admitted exponent
            sign(n // 4) * np.ldexp(rng.uniform(0.5, 1.0, n // 4), rng.integers(-128, -123, n // 4)),  # either side of the floor
            sign(n // 4) * np.ldexp(rng.uniform(0.5, 1.0, n // 4), rng.integers(126, 131, n // 4))]    # either side of the ceiling
    dens = np.concatenate(dens)
    nums = np.where(rng.random(dens.size) < 0.5, rng.uniform(-2000.0, 2000.0, dens.size),
                    sign(dens.size) * np.ldexp(rng.uniform(0.5, 1.0, dens.size), rng.integers(-893, 500, dens.size)))
    # the edges of both operands against each other
    floor, ceil = 2.0 ** -126 - 2.0 ** -150, float(np.nextafter(np.float64(FLT_MAX) + 2.0 ** 103, 0.0))
    ones = [float(np.nextafter(x, 0.0)) for x in (2.0 ** -126, 2.0 ** -30, 0.5, 1.0, 2.0, 2.0 ** 60)]  # fraction bits all ones
    e_den = [floor, float(np.nextafter(floor, 1.0)), 2.0 ** -126, 1e-30, 1e-7, 0.3, 1.0, float(np.nextafter(1.0, 2.0)), 3.0, 1e30, 2.0 ** 127,
             ceil] + ones
    e_num = [0.0, 5e-324, 2.0 ** -1022, 2.0 ** -969, float(np.nextafter(NUM_LOW, 0.0)), NUM_LOW, 2.0 ** -893, 1e-200, 1e-30, 0.75, 1.0,
             float(np.nextafter(1.0, 2.0)), 3.0, 1999.9999999, 2e3, 1e150, float(np.nextafter(NUM_HIGH, 0.0))] + [2.0 ** k for k in range(-8, 12)]
    ed, en = np.meshgrid(e_den, e_num)
    ed, en = ed.ravel(), en.ravel()
    ed = np.concatenate([ed, -ed, ed, -ed])
    en = np.concatenate([en, en, -en, -en])
    # outside the predicate: only the votes' answer is looked at
    out = np.array([0.0, -0.0, 5e-324, -5e-324, 2.0 ** -1022, 1e-300, 2.0 ** -149, 2.0 ** -127, float(np.nextafter(floor, 0.0)),
                    -float(np.nextafter(floor, 0.0)), float(np.nextafter(ceil, np.inf)), -float(np.nextafter(ceil, np.inf)), 2.0 ** 128, 1e300,
                    -1e300, np.inf, -np.inf, np.nan])
    out = np.concatenate([out, sign(20000) * np.ldexp(rng.uniform(0.5, 1.0, 20000), rng.integers(-1073, -127, 20000)),
                          sign(20000) * np.ldexp(rng.uniform(0.5, 1.0, 20000), rng.integers(130, 1024, 20000))])
    assert not _host_admits(out).any()
    den = np.concatenate([dens, ed, out])
    num = np.concatenate([nums, en, rng.uniform(-2000.0, 2000.0, out.size)])
    perm = rng.permutation(den.size)  # admitted and refused lanes side by side in every wave
    return num[perm], den[perm]


def test_unscaled_division_and_votes_on_the_device(flux):
    num, den = _pairs()
    unscaled, quotient, admit = flux.debug_plane_div(num, den)
    want = _host_admits(den)
    in_range = want & (np.abs(num) >= NUM_LOW) & (np.abs(num) < NUM_HIGH)
    small = want & (np.abs(num) < NUM_LOW)
    differ = _bits(unscaled) != _bits(quotient)
    with np.errstate(all="ignore"):
        host = num / den
    print(f"{den.size} pairs: {int(want.sum())} admitted ({int(in_range.sum())} with a num in range, {int(small.sum())} with a smaller one), "
          f"{int((~want).sum())} refused; in range, unscaled != device quotient in {int((differ & in_range).sum())}; "
          f"device quotient != host quotient in {int((_bits(quotient) != _bits(host))[in_range].sum())}; "
          f"smaller nums bit-equal in {int((~differ & small).sum())} of {int(small.sum())}")
    assert den.size >= 180000 and in_range.sum() >= 120000 and small.sum() >= 100 and (~want).sum() >= 40000
    assert np.array_equal((admit & 1) != 0, want)  # the predicate as a function of the lane
    assert np.array_equal((admit & 2) != 0, want)  # ... and as the lane mask the votes take
    bad = np.flatnonzero(differ & in_range)
    assert bad.size == 0, [(float(num[k]).hex(), float(den[k]).hex(), float(unscaled[k]).hex(), float(quotient[k]).hex()) for k in bad[:5]]
    for form in (unscaled, quotient):  # a smaller num: the plane is missed in both forms
        assert np.all(np.abs(form[small]) < SMALL)


def _grazing(flux, base):
    """demo2 seen from a hair above the floor, looking along it."""
    sd = copy.deepcopy(base)
    floor = next(s for s in sd.shapes if isinstance(s, flux.PlaneData))
    assert tuple(floor.normal) == (0.0, 1.0, 0.0)
    cs = sd.camera_settings
    y = floor.point[1] + 1e-3
    cs.eye = (cs.eye[0], y, cs.eye[2])
    cs.look_at = (cs.look_at[0], y, cs.look_at[2])
    cs.up = (0.0, 1.0, 0.0)
    return sd


_oracle = {}   # the oracle's frame and statistics of a case: read under every switch


def _check(flux, oracle_mod, switches, sd, key, root, depth):
    want, o_stats = sc.references(_oracle, key, flux, oracle_mod, sd, root, depth, SEED, kernels=())
    for env in KERNELS:
        # (plain: the frame of the instantiation without statistics, the benchmark's, before the one that counts)
        switches(**env)
        got, gs, plan, _, plain = sc.render(flux, sd, root, depth, SEED, flux.KERNEL_SPLIT, plain=True)
        switches(FLUX_PLANE_AXIS="0", **env)
        general, es, plan_general, _, plain_general = sc.render(flux, sd, root, depth, SEED, flux.KERNEL_SPLIT, plain=True)
        switches()
        assert plan == plan_general and plan["kernel"] == flux._lib.PLAN_SPLIT
        err = float(np.abs(got - want).max())
        print(f"{key} {env}: |split - oracle| {err:.3e}  bits equal to the general form: {np.array_equal(got, general)}  "
              f"segments {gs['segments']}")
        assert np.array_equal(got, general)
        assert np.array_equal(plain, plain_general)
        assert np.array_equal(plain, got)
        assert gs == es, (gs, es)
        assert {k: gs[k] for k in o_stats} == o_stats


@pytest.mark.parametrize("job", JOBS, ids=lambda j: f"root{j[0]}_depth{j[1]}")
@pytest.mark.parametrize("turn", list(TURNS))
def test_frames_equal_the_general_form(flux, oracle_mod, demo2, switches, turn, job):
    root, depth = job
    sd = sc.turned(flux, small_scene(demo2, 8, 6), TURNS[turn])
    plane = next(s for s in sd.shapes if isinstance(s, flux.PlaneData))
    assert sorted(abs(c) for c in plane.normal) == [0.0, 0.0, 1.0]
    _check(flux, oracle_mod, switches, sd, (turn, root, depth), root, depth)


@pytest.mark.parametrize("job", ((16, 5), (23, 5)), ids=lambda j: f"root{j[0]}_depth{j[1]}")
def test_grazing_camera_equals_the_general_form(flux, oracle_mod, demo2, switches, job):
    root, depth = job
    sd = _grazing(flux, small_scene(demo2, 8, 6))
    _check(flux, oracle_mod, switches, sd, ("grazing", root, depth), root, depth)
