"""Box shapes (extension: axis-aligned boxes, include/flux_abi.h FLUX_SHAPE_BOX) on the CPU: the Python and C++ loaders agree on
scenes/box_room.yml down to the flux_shape bits, both reject bad corners with the field's path and take a missing `invert` as
false, the constant agrees across the header, the ctypes mirror and INTEGRATION.md, the frozen CPU checker refuses a box, the C
ABI validates the corners before it looks for a device, the host scene build gives every box six face records (the C++ selftest,
run once more under AddressSanitizer and UBSan), and tests/box_spec.py agrees with a brute-force six-plane evaluation."""
import copy
import math
import os
import re

import numpy as np
import pytest
import yaml

import box_spec
import selftest as st
from conftest import ROOT, SCENES
from extension_checks import cpp_shapes, shape_fields

BOX_SCENE = os.path.join(SCENES, "box_room.yml")


def _build_selftest(exe, extra=()):
    """tests/box_host_selftest.cpp against the C++ host layer and the host scene build (CPU only: no compute call)."""
    return st.build(exe, "box_host_selftest.cpp", csrc=("scene_build.cpp", "bvh.cpp", "launch_plan.cpp"), flags=extra)


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    return st.run(_build_selftest(str(tmp_path_factory.mktemp("box") / "box_host_selftest")), SCENES)


def test_cpp_selftest(selftest):
    for name in ("abi scene", "yaml corners", "cbor round trip", "host scene build", "box-free scene"):
        assert f"ok {name}" in selftest
    assert "all ok" in selftest


def test_cpp_selftest_under_asan_and_ubsan(tmp_path):
    """The same program as a stand-alone sanitized executable: the loaders, the codecs and the host scene build it calls are
    compiled into it with -fsanitize=address,undefined."""
    exe = _build_selftest(str(tmp_path / "box_host_selftest_san"), st.SANITIZE)
    assert "all ok" in st.run(exe, SCENES, env=st.sanitize_env())


def test_both_loaders_give_the_same_flux_shapes(flux, selftest):
    from flux_amd.scene import SceneDesc
    sd = flux.load_scene(BOX_SCENE)
    kinds = [type(s).__name__ for s in sd.shapes]
    assert kinds == ["BoxData", "DiskData", "BoxData", "BoxData", "SphereData"]
    assert sd.shapes[0].invert is True and sd.shapes[2].invert is False  # the second has no `invert` key
    assert sd.shapes[0].corner0 == (-8.0, 0.0, -10.0) and sd.shapes[0].corner1 == (8.0, 8.0, 8.0)
    assert not any(isinstance(s.material, flux.DielectricData) for s in sd.shapes)  # no glass: the hit queue applies
    assert isinstance(sd.shapes[2].material, flux.MatteData) and isinstance(sd.shapes[3].material, flux.GlossyReflectiveData)
    desc = SceneDesc(sd)
    assert desc.desc.num_shapes == 5 and desc.shapes[0].kind == flux._lib.SHAPE_BOX and desc.shapes[0].invert == 1
    cpp = cpp_shapes(selftest)
    assert sorted(cpp) == list(range(5))
    for i in range(5):
        py = shape_fields(desc.shapes[i])
        assert py == cpp[i], (i, py, cpp[i])  # %.17g round-trips every double exactly


def _doc():
    with open(BOX_SCENE) as f:
        return yaml.safe_load(f)


@pytest.mark.parametrize("field,value,msg", [
    ("corner0", None, "shapes[2].Box: missing field `corner0`"), ("corner1", None, "shapes[2].Box: missing field `corner1`"),
    ("corner0", "low", "shapes[2].Box.corner0"), ("corner1", [1.0, 2.0], "shapes[2].Box.corner1"),
    ("corner0", [float("nan"), 0.0, 1.0], "shapes[2].Box.corner0"), ("corner0", [-5.0, float("-inf"), 1.0], "shapes[2].Box.corner0"),
    ("corner1", [-1.5, float("nan"), 4.5], "shapes[2].Box.corner1"), ("corner1", [-1.5, 2.0, float("inf")], "shapes[2].Box.corner1"),
    ("corner1", [-5.0, 2.0, 4.5], "shapes[2].Box.corner1"), ("corner1", [-1.5, 0.0, 4.5], "shapes[2].Box.corner1"),
    ("corner1", [-1.5, 2.0, 0.5], "shapes[2].Box.corner1"), ("invert", 3, "shapes[2].Box.invert")])
def test_python_loader_rejects_bad_boxes(flux, field, value, msg):
    d = _doc()
    body = d["shapes"][2]["Box"]
    if value is None:
        del body[field]
    else:
        body[field] = value
    with pytest.raises(flux.SceneError, match=re.escape(msg)):
        flux.scene_from_dict(d)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_python_loader_names_the_axis(flux, axis):
    d = _doc()
    c1 = list(d["shapes"][2]["Box"]["corner1"])
    c1[axis] = d["shapes"][2]["Box"]["corner0"][axis]  # equal is not above
    d["shapes"][2]["Box"]["corner1"] = c1
    with pytest.raises(flux.SceneError, match=re.escape("shapes[2].Box.corner1") + ".*axis " + "xyz"[axis]):
        flux.scene_from_dict(d)


def test_python_loader_optional_invert_and_unknown_variant(flux):
    d = _doc()
    assert "invert" not in d["shapes"][2]["Box"]
    d["shapes"][2]["Box"]["invert"] = True
    assert flux.scene_from_dict(d).shapes[2].invert is True
    d["shapes"][2] = {"Quad": d["shapes"][2]["Box"]}
    with pytest.raises(flux.SceneError, match="unknown variant `Quad`.*`Disk`, `Box`"):
        flux.scene_from_dict(d)


def test_shape_box_constant_agrees_everywhere(flux):
    hdr = open(os.path.join(ROOT, "include", "flux_abi.h")).read()
    assert int(re.search(r"#define FLUX_SHAPE_BOX (\d+)", hdr).group(1)) == flux._lib.SHAPE_BOX == 3
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert int(re.search(r"pub const FLUX_SHAPE_BOX: i32 = (\d+);", md).group(1)) == 3
    dev = open(os.path.join(ROOT, "flux_amd", "csrc", "flux_device.h")).read()
    assert int(re.search(r"constexpr int kShapeBox = (\d+);", dev).group(1)) == 3
    assert int(re.search(r"#define FLUX_ABI_VERSION (\d+)", hdr).group(1)) == 3  # no version bump: kind 3 is the probe
    assert "BoxData" in flux.__all__


def test_oracle_refuses_a_box(flux, oracle_mod):
    """The frozen checker knows Sphere and Plane only and reads `point` from anything else: a BoxData makes it raise."""
    sd = flux.load_scene(BOX_SCENE)
    with pytest.raises(AttributeError):
        oracle_mod.Oracle(sd, flux.JobConfiguration(1, 2, 50), seed=1)


def test_abi_validates_the_corners_before_the_device(flux):
    """flux_ctx_create: a corner that is not finite, or corner0 >= corner1 on any axis, is FLUX_E_INVALID whatever the machine, with
    the shape index and the axis in the message; a valid box passes validation (then renders, or -- on a machine without a GPU --
    fails with FLUX_E_DEVICE, never FLUX_E_INVALID)."""
    base = flux.load_scene(BOX_SCENE)
    base.output_settings.image_width, base.output_settings.image_height = 8, 6
    cfg = flux.JobConfiguration(1, 2, 50)
    for axis in range(3):
        for which, bad in (("corner0", math.nan), ("corner0", -math.inf), ("corner1", math.inf), ("corner1", math.nan), ("corner1", None)):
            sd = copy.deepcopy(base)
            c = list(getattr(sd.shapes[3], which))
            c[axis] = sd.shapes[3].corner0[axis] if bad is None else bad
            setattr(sd.shapes[3], which, tuple(c))
            with pytest.raises(flux.FluxError) as ei:
                flux.Renderer(sd, cfg)
            assert ei.value.code == flux._lib.E_INVALID, (axis, which, bad, str(ei.value))
            assert "shape 3" in str(ei.value) and "axis " + "xyz"[axis] in str(ei.value), str(ei.value)
    try:
        flux.Renderer(base, cfg).close()
    except flux.FluxError as e:
        assert e.code == flux._lib.E_DEVICE, str(e)


# ---- the spec against six planes ------------------------------------------------------------------------------------------

C0, C1 = (-0.7, 0.2, -1.1), (0.9, 1.5, 0.4)


def spec_rays(rng, count):
    """The GPU test's ray distribution (tests/test_gpu_box.py): origins outside and inside the box, directions aimed at points in
    and around it or random, not unit vectors; plus rays parallel to each axis, rays starting on a face, and rays with the origin
    ON a slab plane and d_k = 0 exactly (the NaN case)."""
    c0, c1 = np.array(C0), np.array(C1)
    ext = c1 - c0
    n = count // 10
    o_out = c0 - 1.5 * ext + rng.uniform(0, 1, (4 * n, 3)) * 4.0 * ext
    o_in = c0 + rng.uniform(0.02, 0.98, (2 * n, 3)) * ext
    o = np.vstack([o_out, o_in])
    target = c0 - 0.3 * ext + rng.uniform(0, 1, (len(o), 3)) * 1.6 * ext
    d = target - o
    k = len(o) // 3
    d[:k] = rng.normal(size=(k, 3))
    d *= rng.uniform(0.5, 2.0, (len(o), 1))
    # parallel to an axis: one or two direction components exactly 0
    op = c0 - 1.0 * ext + rng.uniform(0, 1, (n, 3)) * 3.0 * ext
    dp = rng.normal(size=(n, 3))
    ax = rng.integers(0, 3, n)
    dp[np.arange(n), ax] = 0.0
    two = rng.uniform(size=n) < 0.3
    dp[np.arange(n)[two], (ax[two] + 1) % 3] = 0.0
    # starting on a face (exactly: the face's coordinate), leaving or entering
    of = c0 + rng.uniform(0.05, 0.95, (n, 3)) * ext
    fa = rng.integers(0, 3, n)
    side = rng.integers(0, 2, n)
    of[np.arange(n), fa] = np.where(side == 1, c1[fa], c0[fa])
    df = rng.normal(size=(n, 3))
    # the NaN case: origin on a slab plane (inside or outside the other slabs), d_k = 0 exactly, either sign of zero
    m = count - len(o) - 2 * n
    on = c0 - 0.5 * ext + rng.uniform(0, 1, (m, 3)) * 2.0 * ext
    na = rng.integers(0, 3, m)
    ns = rng.integers(0, 2, m)
    on[np.arange(m), na] = np.where(ns == 1, c1[na], c0[na])
    dn = rng.normal(size=(m, 3))
    dn[np.arange(m), na] = np.where(rng.uniform(size=m) < 0.5, 0.0, -0.0)
    kinds = np.concatenate([np.zeros(len(o), int), np.ones(n, int), np.full(n, 2), np.full(m, 3)])
    return np.vstack([o, op, of, on]), np.vstack([d, dp, df, dn]), kinds


def test_spec_against_six_planes():
    rng = np.random.default_rng(21)
    o, d, kinds = spec_rays(rng, 100000)
    for invert in (False, True):
        hit, t, n, face, (t0, t1, tmin, tmax) = box_spec.box_hit(C0, C1, o, d, invert)
        bh, bt, bn, bface = box_spec.brute_force(C0, C1, o, d, invert)
        gen = (kinds != 3) & ~box_spec.rounding_level(t0, t1, tmin, tmax)  # away from ties and from the NaN case
        assert gen.sum() > 75000 and hit[gen].sum() > 30000 and (~hit[gen]).sum() > 10000
        assert np.array_equal(hit[gen], bh[gen])
        h = gen & hit
        assert np.allclose(t[h], bt[h], rtol=1e-13, atol=0)  # 1/d then a product against one division: an ulp or two
        assert np.array_equal(face[h], bface[h]) and np.array_equal(n[h], bn[h])
        assert set(np.unique(face[h])) == set(range(6))
        inside = np.all((o > np.array(C0)) & (o < np.array(C1)), axis=1)
        gi = gen & inside  # from inside: the exit, unless it lies within T_MIN
        assert np.array_equal(hit[gi], t1[gi] > box_spec.T_MIN) and hit[gi].mean() > 0.99 and gi.sum() > 15000
        out_n = np.sum(n * d, axis=1) * (-1.0 if invert else 1.0)
        assert np.all(out_n[h & inside] > 0) and np.all(out_n[h & ~inside & (t0 > box_spec.T_MIN)] < 0)  # an entry faces the ray


def test_spec_nan_case_written_out():
    """A ray parallel to a slab with its origin ON one of the slab's planes: x or y -- the slab bounds nothing, the ray is judged by
    the other two slabs; z -- a miss, whatever the rest."""
    c0, c1 = np.array(C0), np.array(C1)
    mid = 0.5 * (c0 + c1)
    for zero in (0.0, -0.0):
        for k in range(3):
            for plane in (c0[k], c1[k]):
                o = mid.copy()
                o[k] = plane
                o[(k + 1) % 3] = c0[(k + 1) % 3] - 1.0  # outside the next slab, aimed through the box
                d = np.zeros(3)
                d[k] = zero
                d[(k + 1) % 3] = 1.0
                hit, t, n, face, _ = box_spec.box_hit(C0, C1, o[None], d[None])
                if k == 2:
                    assert not hit[0]
                else:
                    assert hit[0] and t[0] == 1.0 and face[0] == 2 * ((k + 1) % 3)


def test_ray_distribution_stays_within_the_exclusion_cap():
    """The FAST comparison of tests/test_gpu_box.py excludes rays whose decision sits at rounding level; they may be at most 1e-3 of
    the rays, and the spec alone must stay within that on the distribution the GPU test uses."""
    o, d, kinds = spec_rays(np.random.default_rng(7), 100000)
    _, _, _, _, (t0, t1, tmin, tmax) = box_spec.box_hit(C0, C1, o, d)
    r = box_spec.rounding_level(t0, t1, tmin, tmax)
    assert r.sum() <= 1e-3 * len(o), r.sum()
    assert [int((kinds == k).sum()) for k in range(4)] == [60000, 10000, 10000, 20000]
