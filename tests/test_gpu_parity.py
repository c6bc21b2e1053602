"""GPU parity: the HIP path (through the C ABI) against the CPU oracle on the same seeded inputs.

Tolerance: BASELINE.json's north_star states 1e-4 per channel at a fixed seed.  Both sides are FP64.
MATH_STRICT keeps the reference's operation order, so the observed difference is ~1e-13 (libm vs OCML
sin/cos/pow differ by ulps); MATH_FAST (the default: FMA contraction + csrc/flux_math.h) differs by
rounding only, ~1e-12.  The tests assert 1e-9 at the 99.9th percentile and 1e-4 (the stated
tolerance) on whole images, in BOTH modes; path statistics (segments, bounces per material, misses)
must equal the oracle's exactly, i.e. no ray/primitive decision differs.
"""
import numpy as np
import pytest

from conftest import max_abs_diff, small_scene
from extension_checks import math_mode, set_sharded_frame

pytestmark = pytest.mark.gpu

TOL_IMAGE = 1e-4   # north_star tolerance (per channel)
TOL_TIGHT = 1e-9   # what FP64 + same operation order actually delivers


MATH_MODES = ["fast", "strict"]


def _pair(flux, oracle_mod, sd, n, D=5, seed=1, math="fast"):
    cfg = flux.JobConfiguration(n, D, 50)
    r = flux.Renderer(sd, cfg, seed=seed)
    r.set_math(math_mode(flux, math))
    return r, oracle_mod.Oracle(sd, cfg, seed=seed)


@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_tables_match_oracle(flux, oracle_mod, demo2, n):
    sd = small_scene(demo2, 40, 30)
    r, o = _pair(flux, oracle_mod, sd, n, D=3)
    # square samples are pure IEEE +,/ on the same draws: bit-exact
    assert np.array_equal(r.table(flux._lib.TABLE_PIXEL), o.pixel_sets())
    # disc / hemisphere go through sin, cos, pow: ulp-level libm differences only
    assert max_abs_diff(r.table(flux._lib.TABLE_DISC), o.disc_sets()) < 1e-14
    assert max_abs_diff(r.table(flux._lib.TABLE_HEMI), o.hemi_sets()) < 1e-14
    for row in (0, 7, 29):
        assert np.array_equal(r.row_perm(row), o.row_perm(row))
    assert max_abs_diff(r.camera_basis(), o.camera_basis()) == 0.0
    r.close()


@pytest.mark.parametrize("scene_name", ["demo1", "demo2"])
@pytest.mark.parametrize("n", [1, 3, 4, 8, 9])
@pytest.mark.parametrize("variant", [1, 2, 3])
@pytest.mark.parametrize("math", MATH_MODES)
def test_image_parity_small(flux, oracle_mod, demo1, demo2, scene_name, n, variant, math):
    sd = small_scene(demo1 if scene_name == "demo1" else demo2, 64, 48)
    r, o = _pair(flux, oracle_mod, sd, n, math=math)
    r.set_kernel(variant)
    got = r.render_frame()
    want = o.render_frame(threads=8)
    assert got.shape == want.shape == (48, 64, 3)
    d = max_abs_diff(got, want)
    assert d < TOL_IMAGE, d
    # report-quality check: typically ~1e-13
    assert np.percentile(np.abs(got - want), 99.9) < TOL_TIGHT
    r.close()


@pytest.mark.parametrize("math", MATH_MODES)
def test_full_width_rows_parity(flux, oracle_mod, demo2, math):
    """Full 800-wide rows of the real demo2 scene (config 3 geometry) at 64 spp."""
    r, o = _pair(flux, oracle_mod, demo2, 8, math=math)
    for (a, b) in [(0, 1), (298, 301), (598, 599)]:
        got = r.render_rows(a, b)
        want = o.render_rows(a, b, threads=8)
        assert max_abs_diff(got, want) < TOL_IMAGE
    r.close()


@pytest.mark.parametrize("math", MATH_MODES)
def test_stats_match_oracle(flux, oracle_mod, demo2, math):
    sd = small_scene(demo2, 64, 48)
    r, o = _pair(flux, oracle_mod, sd, 8, math=math)
    for variant in (1, 2, 3):
        r.set_kernel(variant)
        r.enable_stats(True)
        r.stats(reset=True)
        r.render_frame()
        o.stats(reset=True)
        o.render_frame(threads=4)
        got = r.stats()
        assert {k: got[k] for k in o.stats()} == o.stats()
    r.close()


def test_work_unit_sharding_invariance(flux, demo2):
    """Rendering the frame as reference work units, single rows or strided rows gives the same pixels
    bit for bit (the per-row permutation is keyed by (seed,row), not by the launch)."""
    sd = small_scene(demo2, 64, 48)
    r = flux.Renderer(sd, flux.JobConfiguration(8, 5, 50), seed=7)
    full = r.render_frame()
    units = flux.work_units(48, 10)
    parts = np.concatenate([r.render(u).rows for u in units], axis=0)
    assert np.array_equal(parts, full[: parts.shape[0]])
    single = np.concatenate([r.render_rows(k, k) for k in range(48)], axis=0)
    assert np.array_equal(single, full)
    again = r.render_frame()
    assert np.array_equal(again, full)  # run-to-run determinism (no atomics)
    r.close()


def test_seed_changes_image(flux, demo2):
    sd = small_scene(demo2, 32, 24)
    a = flux.Renderer(sd, flux.JobConfiguration(4, 5, 50), seed=1).render_frame()
    b = flux.Renderer(sd, flux.JobConfiguration(4, 5, 50), seed=2).render_frame()
    assert not np.array_equal(a, b)
    assert abs(a.mean() - b.mean()) < 0.05


@pytest.mark.parametrize("D", [1, 2, 7])
@pytest.mark.parametrize("math", MATH_MODES)
def test_depth_limits(flux, oracle_mod, demo1, D, math):
    sd = small_scene(demo1, 32, 24)
    r, o = _pair(flux, oracle_mod, sd, 4, D=D, math=math)
    assert max_abs_diff(r.render_frame(), o.render_frame(threads=4)) < TOL_IMAGE
    r.close()


def test_empty_scene_and_background(flux, oracle_mod, demo1):
    import copy
    sd = small_scene(demo1, 16, 8)
    sd = copy.deepcopy(sd)
    sd.shapes = []
    sd.background = (0.25, 0.5, 2.0)  # exercises max_to_one on the background path
    r, o = _pair(flux, oracle_mod, sd, 2)
    got = r.render_frame()
    assert max_abs_diff(got, o.render_frame()) == 0.0
    assert np.allclose(got, np.array([0.125, 0.25, 1.0]))
    r.close()


@pytest.mark.parametrize("math", MATH_MODES)
def test_reflective_and_tie_break(flux, oracle_mod, demo1, math):
    """PerfectSpecular (unused by the demos but part of the schema) and coincident shapes
    (lowest YAML index wins, scene.rs:156-160)."""
    import copy
    sd = copy.deepcopy(small_scene(demo1, 48, 36))
    s = sd.shapes
    s[2].material = flux.ReflectiveData(0.8, (0.9, 0.9, 1.0))
    twin = copy.deepcopy(s[1])
    twin.material = flux.EmissiveData((1.0, 0.0, 0.0), 5.0)
    s.insert(2, twin)  # same centre/radius as shape 1, later in order: must never be seen
    r, o = _pair(flux, oracle_mod, sd, 4, math=math)
    got, want = r.render_frame(), o.render_frame(threads=4)
    assert max_abs_diff(got, want) < TOL_IMAGE
    r.close()


def test_deep_paths(flux, oracle_mod, demo1):
    """max_trace_depth far beyond the default: FAST has no per-depth on-chip state; STRICT's LDS recursion
    stack has a documented limit and fails loudly beyond it."""
    sd = small_scene(demo1, 16, 12)
    r, o = _pair(flux, oracle_mod, sd, 4, D=40, math="fast")
    assert max_abs_diff(r.render_frame(), o.render_frame(threads=4)) < TOL_IMAGE
    r.set_math(flux.MATH_STRICT)
    with pytest.raises(flux.FluxError):
        r.render_frame()
    r.close()
    r, o = _pair(flux, oracle_mod, sd, 4, D=24, math="strict")
    assert max_abs_diff(r.render_frame(), o.render_frame(threads=4)) < TOL_IMAGE
    r.close()


def test_abi_errors(flux, demo1):
    sd = small_scene(demo1, 16, 8)
    with pytest.raises(flux.FluxError):
        flux.Renderer(sd, flux.JobConfiguration(0, 5, 50))
    with pytest.raises(flux.FluxError):
        flux.Renderer(sd, flux.JobConfiguration(2, 0, 50))
    with pytest.raises(flux.FluxError):
        flux.Renderer(sd, flux.JobConfiguration(2, 5, 50), device=99)
    with pytest.raises(flux.FluxError):
        flux.Renderer(sd, flux.JobConfiguration(4096, 8, 50))   # depth * spp beyond the 32-bit table offsets
    r = flux.Renderer(sd, flux.JobConfiguration(2, 5, 50))
    with pytest.raises(flux.FluxError):
        r.render_rows(0, 8)      # row_end == H is out of range
    with pytest.raises(flux.FluxError):
        r.render_rows(5, 4)
    assert r.render_rows(7, 7).shape == (1, 16, 3)
    r.close()
    with pytest.raises(flux.FluxError):
        r.render_rows(0, 0)      # closed


@pytest.mark.parametrize("name", ["demo1", "demo2"])
@pytest.mark.parametrize("math", MATH_MODES)
def test_gpu_matches_committed_golden(flux, demo1, demo2, name, math):
    """tests/golden/*_64x48_n4_seed1.npy (oracle renders committed with their generating script)."""
    import os
    from conftest import GOLDEN
    sd = small_scene(demo1 if name == "demo1" else demo2, 64, 48)
    want = np.load(os.path.join(GOLDEN, f"{name}_64x48_n4_seed1.npy"))
    with flux.Renderer(sd, flux.JobConfiguration(4, 5, 50), seed=1) as r:
        r.set_math(math_mode(flux, math))
        assert max_abs_diff(r.render_frame(), want) < TOL_IMAGE


@pytest.mark.parametrize("math", MATH_MODES)
def test_full_size_properties(flux, demo2, math):
    """BASELINE config geometry (800x600 demo2) at a size the oracle would not finish in seconds
    (1024 spp on a band of rows): size-independent properties instead of a CPU comparison --
    bitwise run-to-run determinism, static == refill up to summation order, strided == contiguous rows,
    all values finite and in [0,1] after max_to_one."""
    with flux.Renderer(demo2, flux.JobConfiguration(32, 5, 50), seed=1) as r:
        r.set_math(math_mode(flux, math))
        a = r.render_rows(296, 303)
        b = r.render_rows(296, 303)
        assert np.array_equal(a, b)
        assert np.isfinite(a).all() and a.min() >= 0.0 and a.max() <= 1.0
        r.set_kernel(flux.KERNEL_STATIC)
        c = r.render_rows(296, 303)
        assert max_abs_diff(a, c) < 1e-12  # same samples, different (fixed) summation order
        r.set_kernel(flux.KERNEL_REFILL)
        r.enable_stats(True)
        r.stats(reset=True)
        r.render_rows(296, 303)
        st = r.stats()
        assert st["samples"] == 8 * 800 * 1024
        assert st["segments"] == st["matte_bounces"] + st["glossy_bounces"] + st["specular_bounces"] + \
            st["emissive_hits"] + st["misses"]
        assert st["misses"] == 0  # demo2 is enclosed by the inverted environment sphere


def test_fast_equals_strict_full_size(flux, demo2):
    """The two arithmetics on the BASELINE geometry at 1024 spp (no oracle at this size): same image
    to rounding and identical path statistics (no hit/miss/material decision differs)."""
    with flux.Renderer(demo2, flux.JobConfiguration(32, 5, 50), seed=1) as r:
        out, stats = {}, {}
        for name in MATH_MODES:
            r.set_math(math_mode(flux, name))
            r.enable_stats(True)
            r.stats(reset=True)
            out[name] = r.render_rows(280, 311)
            stats[name] = r.stats(reset=True)
        assert stats["fast"] == stats["strict"]
        assert max_abs_diff(out["fast"], out["strict"]) < 1e-9


@pytest.mark.parametrize("math", MATH_MODES)
def test_gpu_matches_reference_published_render(flux, demo2, math):
    """The reference's only published output -- demo.png: demo2.yml at 16384 spp (README.md:1-3), committed
    as 8x8 box-filtered means (tests/golden/make_demo2_ref.py) -- against the GPU render of the same scene
    at the same 16384 spp.  Different RNG (the reference seeds from OS entropy) and an 8-bit source, so the
    bound is quantisation (1/255 = 0.0039 per source pixel) + residual noise, not equality.  Measured: mean |d|
    0.00126, 99th percentile 0.0033, max 0.0057, per-channel bias <= 0.0009."""
    import os
    from conftest import GOLDEN
    ref = np.load(os.path.join(GOLDEN, "demo2_ref_100x75.npy")).astype(np.float64)
    with flux.Renderer(demo2, flux.JobConfiguration(128, 5, 50), seed=1) as r:
        r.set_math(math_mode(flux, math))
        img = r.render_frame()
    assert np.isfinite(img).all() and img.min() >= 0.0 and img.max() <= 1.0
    small = img.reshape(75, 8, 100, 8, 3).mean(axis=(1, 3))
    d = small - ref
    assert np.abs(d).mean() < 0.0025, np.abs(d).mean()
    assert np.all(np.abs(d.mean(axis=(0, 1))) < 0.0015), d.mean(axis=(0, 1))  # no colour bias
    assert np.percentile(np.abs(d), 99) < 0.008 and np.abs(d).max() < 0.02
    assert small[:20, 60:].mean() > small[:20, :40].mean()  # glow top-right, far spheres top-left


@pytest.mark.parametrize("math", MATH_MODES)
@pytest.mark.parametrize("variant", [1, 2, 3])
def test_many_shapes_batches_and_planes(flux, oracle_mod, demo1, math, variant):
    """More shapes than one 32-wide candidate batch (75 spheres incl. nested/overlapping/coincident ones,
    4 planes interleaved in YAML order, every material kind): the sphere scan's batching, the plane/sphere
    tie rule and the hit-record indirection against the oracle's linear scan."""
    import copy
    rng = np.random.default_rng(42)
    sd = copy.deepcopy(small_scene(demo1, 48, 36))
    shapes = [sd.shapes[0]]  # the inverted environment sphere
    mats = [lambda: flux.MatteData((rng.uniform(), rng.uniform(), rng.uniform()), (0, 0, 0), rng.uniform(0.3, 1.0)),
            lambda: flux.EmissiveData((rng.uniform(), rng.uniform(), rng.uniform()), rng.uniform(0.5, 3.0)),
            lambda: flux.ReflectiveData(rng.uniform(0.3, 0.9), (rng.uniform(), rng.uniform(), rng.uniform())),
            lambda: flux.GlossyReflectiveData(rng.uniform(0.3, 0.9), (rng.uniform(), rng.uniform(), rng.uniform()),
                                              float(rng.choice([3.0, 10.0, 101.0, 1000.5])))]
    for k in range(74):
        c = (rng.uniform(-4, 9), rng.uniform(0.2, 3.0), rng.uniform(-3, 12))
        s = flux.SphereData(c, float(rng.uniform(0.2, 1.2)), mats[k % 4](), bool(k % 17 == 5))
        shapes.append(s)
        if k % 20 == 7:
            shapes.append(copy.deepcopy(s))  # coincident twin later in the order: never visible
            shapes[-1].material = flux.EmissiveData((9.0, 0.0, 9.0), 50.0)
        if k % 19 == 3:
            n = (rng.uniform(-0.2, 0.2), 1.0, rng.uniform(-0.2, 0.2))
            shapes.append(flux.PlaneData((0.0, rng.uniform(-0.5, 0.1), 0.0), n, mats[(k // 19) % 4]()))
    sd.shapes = shapes
    assert sum(isinstance(s, flux.SphereData) for s in shapes) > 64 and sum(isinstance(s, flux.PlaneData) for s in shapes) == 4
    r, o = _pair(flux, oracle_mod, sd, 4, math=math)
    r.set_kernel(variant)
    r.enable_stats(True)
    r.stats(reset=True)
    got = r.render_frame()
    o.stats(reset=True)
    want = o.render_frame(threads=8)
    st = r.stats()
    assert {k: st[k] for k in o.stats()} == o.stats()
    assert max_abs_diff(got, want) < TOL_IMAGE
    r.close()


@pytest.mark.parametrize("math", MATH_MODES)
@pytest.mark.parametrize("world", [1, 3, 8])
def test_set_sharded_render_equals_full_frame(flux, demo2, math, world):
    """flux_render_sets_device: the G per-rank shares (sets s % G == g), rendered one after the other on this one
    GPU and reassembled by SetSharder's indexing, give the bit-identical frame of the row-based render."""
    import torch
    from flux_amd.dist import SetSharder
    sd = small_scene(demo2, 40, 24)
    with flux.Renderer(sd, flux.JobConfiguration(8, 5, 50), seed=3) as r:
        r.set_math(math_mode(flux, math))
        full = torch.from_numpy(r.render_frame())
        assert torch.equal(set_sharded_frame(flux, r, world), full)
        s0 = SetSharder(24, 40, 0, world, torch.device("cuda", 0), torch.from_numpy(r.row_perm_table()))
        with pytest.raises(flux.FluxError):
            r.render_sets_device(0, 1, 41, s0.render_buf.data_ptr())   # more sets than exist
        r.set_kernel(flux.KERNEL_STATIC)
        with pytest.raises(flux.FluxError):
            r.render_sets_device(0, 1, 40, s0.render_buf.data_ptr())   # needs the refill kernel


@pytest.mark.parametrize("lens,focal,pixel", [(5.0, 3.0, 6.0), (0.9, 1.0, 40.0), (0.0, 10.0, 400.0)])
def test_split_kernel_with_extreme_cameras(flux, oracle_mod, demo2, lens, focal, pixel):
    """The split kernel's per-pixel candidate mask (pixel_sphere_mask) must stay a superset of what any primary ray of
    the pixel can hit, also for ray bundles that are anything but narrow: a lens wider than the focal distance (the
    bundle's cone opens beyond 45 degrees), and pixels whose footprint spans the whole scene.  Path statistics equal to the
    oracle's mean no hit was missed."""
    import copy
    sd = copy.deepcopy(small_scene(demo2, 24, 18))
    sd.camera_data.lens_radius = lens
    sd.camera_data.focal_distance = focal
    sd.output_settings.pixel_size = pixel
    cfg = flux.JobConfiguration(16, 5, 50)   # 256 spp: the split kernel's range
    o = oracle_mod.Oracle(sd, cfg, seed=9)
    o.stats(reset=True)
    want = o.render_frame(threads=8)
    with flux.Renderer(sd, cfg, seed=9) as r:
        r.set_kernel(flux.KERNEL_SPLIT)
        r.enable_stats(True)
        r.stats(reset=True)
        got = r.render_frame()
        st = r.stats()
    assert {k: st[k] for k in o.stats()} == o.stats()
    assert max_abs_diff(got, want) < TOL_IMAGE


def _env_cases(flux, demo2):
    """Scenes around the two FAST scan shortcuts: `invert` spheres tested for all lanes at once (ties with a coincident
    convex twin in either YAML order, three nested environments, a camera outside an environment) and rays that leave a
    convex sphere outwards skipping that sphere (a camera INSIDE a big convex sphere of every sampled material, so hits come
    from inside too; a sphere beyond the 1e3 magnitude guard, which switches the shortcut off for the scene)."""
    import copy
    base = copy.deepcopy(small_scene(demo2, 24, 18))
    env = next(s for s in base.shapes if isinstance(s, flux.SphereData) and s.invert)
    rest = [s for s in base.shapes if s is not env]
    cases = {}
    for order in ("convex_first", "inverted_first"):
        sd = copy.deepcopy(base)
        twin = flux.SphereData(tuple(env.center), float(env.radius), flux.EmissiveData((0.2, 0.9, 0.3), 2.0), False)
        e = copy.deepcopy(env)
        sd.shapes = ([twin, e] if order == "convex_first" else [e, twin]) + copy.deepcopy(rest)
        cases[order] = sd
    sd = copy.deepcopy(base)
    e2, e3 = copy.deepcopy(env), copy.deepcopy(env)
    e2.radius, e3.radius = float(env.radius) * 0.5, float(env.radius) * 0.25
    e2.material = flux.MatteData((0.7, 0.8, 0.9), (0, 0, 0), 0.8)
    e3.material = flux.GlossyReflectiveData(0.7, (0.9, 0.8, 0.7), 30.0)
    sd.shapes = copy.deepcopy(rest[:3]) + [e3] + copy.deepcopy(rest[3:]) + [e2, copy.deepcopy(env)]
    cases["nested_environments"] = sd
    sd = copy.deepcopy(base)
    small_env = copy.deepcopy(env)
    small_env.center, small_env.radius = (0.0, 1.0, 0.0), 4.0   # the camera (10 away) looks at it from outside
    small_env.material = flux.EmissiveData((0.9, 0.9, 0.5), 1.5)
    sd.shapes = [small_env] + copy.deepcopy(rest)
    cases["camera_outside_environment"] = sd
    mats = {"matte": flux.MatteData((0.8, 0.7, 0.6), (0, 0, 0), 0.9),
            "glossy": flux.GlossyReflectiveData(0.8, (0.9, 0.9, 0.8), 20.0),
            "reflective": flux.ReflectiveData(0.85, (0.9, 0.95, 1.0))}
    for name, m in mats.items():
        sd = copy.deepcopy(base)
        shell = flux.SphereData((0.0, 0.0, 0.0), 40.0, m, False)     # convex, seen from inside
        sd.shapes = [shell] + copy.deepcopy(rest)                      # no environment: paths that get out miss
        cases["inside_convex_" + name] = sd
    sd = copy.deepcopy(base)
    sd.shapes = copy.deepcopy(base.shapes) + [flux.SphereData((0.0, 1504.0, 0.0), 1500.0, mats["matte"], False)]
    cases["beyond_the_magnitude_guard"] = sd
    # the split kernel's square-root-free decision for an Emissive environment (RenderParams::env_short): surfaces that
    # meet the environment sphere, so that "nearer than the best hit so far" is decided at and around equality, and
    # bounce origins closer to it than its margin -- the cases its fallback to the exact code exists for
    R, c = float(env.radius), tuple(float(x) for x in env.center)
    sd = copy.deepcopy(base)
    sd.shapes = [s for s in copy.deepcopy(base.shapes) if not isinstance(s, flux.PlaneData)] + [
        flux.PlaneData((c[0], c[1] - R + 0.02, c[2]), (0.0, 1.0, 0.0), mats["matte"])]   # cuts a cap of radius 2 off its lowest point
    sd.camera_settings.eye, sd.camera_settings.look_at = (c[0], c[1] - R + 3.0, c[2] - 6.0), (c[0], c[1] - R, c[2])
    cases["plane_tangent_to_the_environment"] = sd
    sd = copy.deepcopy(base)
    sd.shapes = copy.deepcopy(base.shapes) + [flux.SphereData((c[0], c[1] + 6.0, c[2] + R - 4.0), 9.0, mats["matte"], False)]  # crosses it
    sd.camera_settings.eye, sd.camera_settings.look_at = (c[0], c[1] + 6.0, c[2] + R - 30.0), (c[0], c[1] + 6.0, c[2] + R)
    cases["sphere_across_the_environment"] = sd
    sd = copy.deepcopy(base)
    sd.shapes = copy.deepcopy(base.shapes) + [flux.SphereData((c[0], c[1] + 2.0, c[2] + R - 1.0001), 1.0, mats["matte"], False),   # 1e-4 short of touching
                                             flux.SphereData((c[0] + 3.0, c[1] + 2.0, c[2] + R - 1.0), 1.0, mats["glossy"], False)]  # touching
    sd.camera_settings.eye, sd.camera_settings.look_at = (c[0] + 1.5, c[1] + 2.0, c[2] + R - 9.0), (c[0] + 1.5, c[1] + 2.0, c[2] + R)
    cases["spheres_touching_the_environment"] = sd
    return cases


@pytest.mark.parametrize("variant", [2, 3])
@pytest.mark.parametrize("case", ["convex_first", "inverted_first", "nested_environments", "camera_outside_environment",
                                  "inside_convex_matte", "inside_convex_glossy", "inside_convex_reflective",
                                  "beyond_the_magnitude_guard", "plane_tangent_to_the_environment",
                                  "sphere_across_the_environment", "spheres_touching_the_environment"])
def test_environment_and_self_leaving_shortcuts(flux, oracle_mod, demo2, case, variant):
    sd = _env_cases(flux, demo2)[case]
    cfg = flux.JobConfiguration(16, 5, 50)   # 256 spp: refill and split kernels
    o = oracle_mod.Oracle(sd, cfg, seed=4)
    o.stats(reset=True)
    want = o.render_frame(threads=8)
    with flux.Renderer(sd, cfg, seed=4) as r:
        r.set_kernel(variant)
        r.enable_stats(True)
        r.stats(reset=True)
        got = r.render_frame()
        st = r.stats()
    assert {k: st[k] for k in o.stats()} == o.stats()
    assert max_abs_diff(got, want) < TOL_IMAGE


def test_fast_means_strict_where_a_plane_normal_is_not_unit(flux, oracle_mod, demo2):
    """FLUX_MATH_FAST is defined for unit surface normals.  A plane stored with a non-unit normal (the reference never
    normalises it, shapes.rs:135-152) makes reflected directions non-unit and Phong lobes under- / overflow; the reference's
    recursion (materials.rs:31-33, 69-71) then meets its zeros and infinities in an order no reordered product reproduces, so
    the library renders such a scene with the STRICT arithmetic whatever the setting: the launch plan says so, and the FAST
    and STRICT frames are the same bits.  The same scene with the normal normalised runs the FAST kernels."""
    import copy
    sd = copy.deepcopy(small_scene(demo2, 48, 36))
    plane = next(s for s in sd.shapes if isinstance(s, flux.PlaneData))
    unit = tuple(float(x) for x in np.array(plane.normal) / np.linalg.norm(plane.normal))
    cfg = flux.JobConfiguration(16, 5, 50)
    frames = {}
    for label, normal in (("unit", unit), ("scaled", tuple(2.5 * x for x in unit))):
        plane.normal = normal
        with flux.Renderer(sd, cfg, seed=5) as r:
            for math in MATH_MODES:
                r.set_math(math_mode(flux, math))
                plan = r.launch_plan()
                want_math = flux.MATH_STRICT if (label == "scaled" or math == "strict") else flux.MATH_FAST
                assert plan["math"] == want_math, (label, math, plan)
                assert plan["kernel"] == (flux._lib.PLAN_SPLIT if want_math == flux.MATH_FAST else flux._lib.PLAN_REFILL)
                frames[(label, math)] = r.render_frame()
        o = oracle_mod.Oracle(sd, cfg, seed=5)
        want = o.render_frame(threads=8)
        finite = np.isfinite(want)
        for math in MATH_MODES:
            got = frames[(label, math)]
            assert np.array_equal(np.isfinite(got), finite)
            assert max_abs_diff(got[finite], want[finite]) < TOL_IMAGE
    assert np.array_equal(frames[("scaled", "fast")], frames[("scaled", "strict")], equal_nan=True)
    assert not np.array_equal(frames[("unit", "fast")], frames[("unit", "strict")])   # two arithmetics: equal to rounding only
    assert max_abs_diff(frames[("unit", "fast")], frames[("unit", "strict")]) < TOL_TIGHT


def test_a_job_too_deep_for_strict_stays_fast_on_a_non_unit_plane(flux, oracle_mod, demo2):
    """STRICT keeps 32 B of recursion stack per level and lane in LDS -- 31 levels at most.  A FAST job deeper
    than that on a scene with a non-unit plane normal used to be routed to STRICT and then REFUSED (it rendered before round 4);
    now the routing is dropped where STRICT cannot run: the launch plan says FAST, the frame comes from FAST's long-form glossy
    weights (RenderParams::glossy_long) and meets the oracle; the same job in explicit STRICT is refused with a message that names
    FLUX_MATH_FAST, and the Renderer warns once where the routing does apply."""
    import copy
    import warnings
    sd = copy.deepcopy(small_scene(demo2, 32, 24))
    plane = next(s for s in sd.shapes if isinstance(s, flux.PlaneData))
    plane.normal = tuple(1.7 * x for x in plane.normal)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with flux.Renderer(sd, flux.JobConfiguration(8, 5, 50), seed=9) as r:      # depth 5: STRICT fits, the routing applies
            assert r.launch_plan()["math"] == flux.MATH_STRICT and "FAST -> STRICT" in repr(r)
            assert r.launch_plan()["route"] == flux._lib.ROUTE_TO_STRICT
        assert sum("non-unit normal" in str(x.message) for x in w) == 1
    cfg = flux.JobConfiguration(16, 40, 50)
    o = oracle_mod.Oracle(sd, cfg, seed=9)
    o.stats(reset=True)
    want = o.render_frame(threads=8)
    ost = o.stats()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with flux.Renderer(sd, cfg, seed=9) as r:
            assert r.launch_plan()["math"] == flux.MATH_FAST and "->" not in repr(r)
            assert r.launch_plan()["route"] == flux._lib.ROUTE_KEPT_FAST      # (said out loud, see the warning below)
            assert r.launch_plan()["kernel"] == flux._lib.PLAN_SPLIT          # 256 spp: the default kernel, long-form glossy weights
            r.enable_stats(True)
            for variant in (flux.KERNEL_DEFAULT, flux.KERNEL_REFILL, flux.KERNEL_STATIC):
                r.set_kernel(variant)
                r.stats(reset=True)
                got = r.render_frame()
                st = r.stats(reset=True)
                assert {k: st[k] for k in ost} == ost, variant
                finite = np.isfinite(want) & np.isfinite(got)
                assert finite.mean() > 0.99 and max_abs_diff(got[finite], want[finite]) < TOL_IMAGE, variant
            r.set_math(flux.MATH_STRICT)
            with pytest.raises(flux.FluxError, match="FLUX_MATH_FAST or a smaller max_trace_depth"):
                r.render_frame()
        # the job that STAYS on FAST although the scene asks for STRICT is reported too, once, in its own words
        kept = [str(x.message) for x in w if "non-unit normal" in str(x.message)]
        assert len(kept) == 1 and "stays on FLUX_MATH_FAST" in kept[0], kept
    with flux.Renderer(small_scene(demo2, 32, 24), cfg, seed=9) as r:              # unit normals: nothing to route, nothing to say
        assert r.launch_plan()["route"] == flux._lib.ROUTE_NONE


def test_routing_to_strict_does_not_depend_on_the_traversal_hook(flux, demo2):
    """the arithmetic a scene is rendered with is a function of the job (max_trace_depth, the mesh's BVH depth), never of
    flux_ctx_set_traversal -- a test hook must not flip the frame.  A mesh scene with a non-unit plane normal at a depth where STRICT's
    recursion stack fits only WITHOUT the BVH stack beside it: before, the brute-force hook made it fit and routed the job to STRICT."""
    import copy
    from flux_amd.procedural import heightfield_scene
    sd = copy.deepcopy(heightfield_scene(24, 16, seed=5, base=small_scene(demo2, 24, 18)))
    plane = next(s for s in sd.shapes if isinstance(s, flux.PlaneData))
    plane.normal = tuple(1.3 * x for x in plane.normal)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with flux.Renderer(sd, flux.JobConfiguration(8, 31, 50), seed=2) as r:
            depth = r.bvh_info()["max_depth"]
            fits = 31 * 4 * 64 * 8 + depth * 64 * 4 + 512 <= 64 * 1024
            plans = {}
            for mode in (flux._lib.TRAVERSE_BVH, flux._lib.TRAVERSE_BRUTE, flux._lib.TRAVERSE_BVH_BINARY):
                r.set_traversal(mode)
                plans[mode] = (r.launch_plan()["math"], r.launch_plan()["route"])
            assert len(set(plans.values())) == 1, plans
            assert plans[flux._lib.TRAVERSE_BVH] == ((flux.MATH_STRICT, flux._lib.ROUTE_TO_STRICT) if fits else
                                                     (flux.MATH_FAST, flux._lib.ROUTE_KEPT_FAST)), (plans, depth)


def test_split_kernel_serves_scenes_with_many_planes(flux, oracle_mod, demo1):
    """the split kernel keeps the scene's records in LDS and used to leave any scene with more than 16 planes to the refill
    kernel without a word.  The rule is now by bytes (records <= 16 KiB): 64 spheres + 20 planes run the split kernel -- and meet the oracle,
    statistics included --, 65 spheres (the pixel mask's width) or 200 planes take the refill kernel, and the launch plan says which."""
    import copy
    rng = np.random.default_rng(7)
    base = copy.deepcopy(small_scene(demo1, 40, 30))

    def scene(n_sph, n_pln):
        sd = copy.deepcopy(base)
        shapes = [sd.shapes[0]]  # the inverted environment sphere
        for k in range(n_sph - 1):
            m = (flux.MatteData((0.6, 0.5, 0.4), (0, 0, 0), 0.8) if k % 3 == 0 else
                 flux.GlossyReflectiveData(0.7, (0.9, 0.8, 0.9), float([10.0, 100.0, 1e4][k % 3])) if k % 3 == 1 else
                 flux.ReflectiveData(0.8, (0.9, 0.9, 1.0)))
            shapes.append(flux.SphereData((float(rng.uniform(-4, 9)), float(rng.uniform(0.2, 3.0)), float(rng.uniform(-3, 12))),
                                          float(rng.uniform(0.2, 0.9)), m, False))
        for k in range(n_pln):  # tilted floors and walls, unit normals (FAST stays FAST)
            n = np.array([rng.uniform(-0.3, 0.3), 1.0, rng.uniform(-0.3, 0.3)])
            n /= np.linalg.norm(n)
            shapes.append(flux.PlaneData((0.0, float(-0.2 - 0.3 * k), 0.0), tuple(float(x) for x in n),
                                         flux.MatteData((0.5, 0.5, 0.5), (1, 1, 1), 1.0)))
        sd.shapes = shapes
        return sd

    cfg = flux.JobConfiguration(16, 5, 50)   # 256 spp: the split kernel's range
    sd = scene(64, 20)
    o = oracle_mod.Oracle(sd, cfg, seed=4)
    o.stats(reset=True)
    want = o.render_frame(threads=8)
    ost = o.stats()
    o.close()
    with flux.Renderer(sd, cfg, seed=4) as r:
        plan = r.launch_plan()
        assert plan["kernel"] == flux._lib.PLAN_SPLIT and plan["math"] == flux.MATH_FAST, plan
        assert plan["lds"] >= (64 + 20) * 96 + 64 * 32
        r.enable_stats(True)
        r.stats(reset=True)
        got = r.render_frame()
        st = r.stats()
        assert {k: st[k] for k in ost} == ost
        assert max_abs_diff(got, want) < TOL_IMAGE
        r.set_kernel(flux.KERNEL_REFILL)
        assert max_abs_diff(r.render_frame(), got) < 1e-12
    for n_sph, n_pln in ((65, 1), (12, 200)):
        with flux.Renderer(scene(n_sph, n_pln), cfg, seed=4) as r:
            assert r.launch_plan()["kernel"] == flux._lib.PLAN_REFILL, (n_sph, n_pln)
            assert np.isfinite(r.render_frame()).all()


def test_filter_walk_and_first_plane_for_every_scene_shape(flux, oracle_mod, demo1):
    """Round 6 moved two pieces of per-pass arithmetic out of the kernels: the f32 filter's walk over a scene of at most 32 spheres
    (half group / full groups / valid-bit mask: abi.hip lays them out, `sphere_filter32_laid_out` follows them) and the first plane of
    the scan (peeled: one compare and one select).  Every remainder of the pair groups -- 1 ... 34 spheres, the last two beyond the
    one-group instantiation -- and 0 / 1 / 3 planes must meet the oracle with identical path statistics, in the split kernel (256 spp)
    and in the refill kernel; with and without an environment sphere (the usual-scene instantiation needs one)."""
    import copy
    rng = np.random.default_rng(11)
    base = copy.deepcopy(small_scene(demo1, 32, 24))
    env = base.shapes[0]  # the inverted environment sphere

    def scene(n_sph, n_pln, with_env):
        sd = copy.deepcopy(base)
        shapes = [env] if with_env else []
        while len(shapes) < n_sph:
            k = len(shapes)
            m = (flux.MatteData((0.6, 0.5, 0.4), (0, 0, 0), 0.8) if k % 4 == 0 else
                 flux.GlossyReflectiveData(0.7, (0.9, 0.8, 0.9), float([10.0, 100.0, 1e4][k % 3])) if k % 4 == 1 else
                 flux.ReflectiveData(0.8, (0.9, 0.9, 1.0)) if k % 4 == 2 else
                 flux.EmissiveData((1.0, 0.9, 0.8), 1.5))
            shapes.append(flux.SphereData((float(rng.uniform(-5, 5)), float(rng.uniform(0.2, 3.0)), float(rng.uniform(-2, 10))),
                                          float(rng.uniform(0.2, 0.8)), m, False))
        for k in range(n_pln):
            n = np.array([rng.uniform(-0.2, 0.2), 1.0, rng.uniform(-0.2, 0.2)])
            n /= np.linalg.norm(n)
            shapes.append(flux.PlaneData((0.0, float(-0.1 - 0.4 * k), 0.0), tuple(float(x) for x in n),
                                         flux.MatteData((0.5, 0.5, 0.5), (1, 1, 1), 1.0)))
        sd.shapes = shapes
        return sd

    cfg = flux.JobConfiguration(16, 5, 50)  # 256 spp: four waves' worth, the split kernel's range
    cases = [(n, 1, True) for n in (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 15, 16, 17, 23, 24, 25, 31, 32, 33, 34)]
    cases += [(6, 0, True), (6, 3, True), (13, 3, True), (5, 1, False), (8, 0, False), (12, 2, False)]
    for n_sph, n_pln, with_env in cases:
        sd = scene(n_sph, n_pln, with_env)
        o = oracle_mod.Oracle(sd, cfg, seed=9)
        o.stats(reset=True)
        want = o.render_frame(threads=8)
        ost = o.stats()
        o.close()
        with flux.Renderer(sd, cfg, seed=9) as r:
            assert r.launch_plan()["math"] == flux.MATH_FAST
            for kern in (flux.KERNEL_DEFAULT, flux.KERNEL_REFILL):
                r.set_kernel(kern)
                r.enable_stats(True)
                r.stats(reset=True)
                got = r.render_frame()
                st = r.stats()
                assert {k: st[k] for k in ost} == ost, (n_sph, n_pln, with_env, kern)
                assert max_abs_diff(got, want) < TOL_IMAGE, (n_sph, n_pln, with_env, kern)
                r.enable_stats(False)
                assert max_abs_diff(r.render_frame(), got) < 1e-12, (n_sph, n_pln, with_env, kern)


def test_strict_filter_equals_the_full_scan(flux, demo1, demo2):
    """Round 5: STRICT takes its sphere candidates from FAST's conservative f32 filter (a sphere the filter rejects is a miss
    whatever BoundingBox::hit says, shapes.rs:173-214) and runs box + quadratic exactly as the reference has them for the rest.
    The frames must be the SAME BITS as with the full scan.  The full scan is still in the library -- it serves scenes the f32
    filter is not defined for (a coordinate beyond 1e15) -- so the same scene with one unreachable sphere at x = 1e16 appended
    (last: nobody's YAML index moves) renders through it: frames and path statistics equal bit for bit, demo1, demo2 and fuzz
    scenes with inverted spheres, coincident twins and non-unit planes, static and refill kernels.
    (Round 5 did the same against a build without the filter: profiles/r05_experiments/strict_filter_check*.log.)"""
    import copy
    from test_gpu_fuzz import random_scene
    scenes = [(small_scene(demo1, 96, 72), 8, 5, 1), (small_scene(demo2, 96, 72), 8, 5, 2)]
    rng = np.random.default_rng(77)
    for case in range(24):
        scenes.append((random_scene(flux, demo1, rng, unit_planes=case % 2 == 1), int(rng.choice([1, 3, 8])), int(rng.choice([1, 5, 9])),
                       int(rng.integers(1, 1 << 30))))
    for sd, n, D, seed in scenes:
        far = copy.deepcopy(sd)
        far.shapes = list(far.shapes) + [flux.SphereData((1.0e16, 0.0, 0.0), 1.0, flux.MatteData((0.5, 0.5, 0.5), (0, 0, 0), 1.0), False)]
        cfg = flux.JobConfiguration(n, D, 50)
        out = []
        for scene in (sd, far):
            with flux.Renderer(scene, cfg, seed=seed) as r:
                r.set_math(flux.MATH_STRICT)
                r.enable_stats(True)
                for variant in (flux.KERNEL_STATIC, flux.KERNEL_REFILL):
                    r.set_kernel(variant)
                    r.stats(reset=True)
                    frame = r.render_frame()
                    out.append((frame, r.stats(reset=True)))
        half = len(out) // 2
        for (fa, sa), (fb, sb) in zip(out[:half], out[half:]):
            assert np.array_equal(fa, fb, equal_nan=True)
            assert sa == sb


def test_strict_fits_its_waves_per_pixel_to_the_recursion_stack(flux, demo2):
    """STRICT keeps 32 B of (f, s) recursion stack per level and lane in LDS.  At 16384 spp four waves share a pixel (K = 4,
    256 lanes): seven levels fit the 64 KiB a block may have.  A deeper job used to be refused; now K falls to what fits (a
    function of the job alone, so the image still does not depend on the sharding) and the frame equals the static kernel's."""
    sd = small_scene(demo2, 8, 6)
    with flux.Renderer(sd, flux.JobConfiguration(128, 9, 50), seed=2) as r:
        r.set_math(flux.MATH_STRICT)
        plan = r.launch_plan()
        assert plan["kernel"] == flux._lib.PLAN_REFILL and plan["waves_per_pixel"] == 2 and plan["lds"] <= 60 * 1024, plan
        a = r.render_frame()
        r.set_kernel(flux.KERNEL_STATIC)
        assert r.launch_plan()["waves_per_pixel"] == 1
        assert max_abs_diff(a, r.render_frame()) < 1e-12
        r.set_kernel(flux.KERNEL_DEFAULT)
        r.set_math(flux.MATH_FAST)            # FAST keeps its throughput in registers: four waves at any depth
        assert r.launch_plan()["waves_per_pixel"] == 4 and r.launch_plan()["math"] == flux.MATH_FAST
        assert max_abs_diff(a, r.render_frame()) < TOL_TIGHT
