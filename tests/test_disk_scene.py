"""Disk shapes (extension: the finite planar area light, include/flux_abi.h FLUX_SHAPE_DISK) on the CPU: the Python and C++
loaders agree on scenes/disk_light.yml down to the flux_shape bits, both reject bad radii with the field's path, the constant
agrees across the header, the ctypes mirror and INTEGRATION.md, the frozen CPU checker refuses a disk instead of rendering an
infinite plane, and the C ABI validates a disk's radius before it looks for a device."""
import copy
import math
import os
import re

import pytest
import yaml

import selftest as st
from conftest import ROOT, SCENES
from extension_checks import cpp_shapes, shape_fields

DISK_SCENE = os.path.join(SCENES, "disk_light.yml")


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    """tests/disk_host_selftest.cpp built against the C++ host layer (CPU only: no compute call)."""
    exe = st.build(str(tmp_path_factory.mktemp("disk") / "disk_host_selftest"), "disk_host_selftest.cpp", host=True, compiler="g++")
    return st.run(exe, SCENES)


def test_cpp_selftest(selftest):
    for name in ("abi scene", "yaml radius", "cbor round trip"):
        assert f"ok {name}" in selftest
    assert "all ok" in selftest


def test_both_loaders_give_the_same_flux_shapes(flux, selftest):
    from flux_amd.scene import SceneDesc
    sd = flux.load_scene(DISK_SCENE)
    assert isinstance(sd.shapes[1], flux.DiskData)
    assert sd.shapes[1].center == (-9.0, 7.0, 8.0) and sd.shapes[1].normal == (0.0, -1.0, 0.0) and sd.shapes[1].radius == 5.0
    desc = SceneDesc(sd)
    assert desc.desc.num_shapes == 13 and desc.shapes[1].kind == flux._lib.SHAPE_DISK
    cpp = cpp_shapes(selftest)
    assert sorted(cpp) == list(range(13))
    for i in range(13):
        py = shape_fields(desc.shapes[i])
        assert py == cpp[i], (i, py, cpp[i])  # %.17g round-trips every double exactly


def test_disk_light_is_demo2_with_the_sphere_light_replaced(flux):
    a, b = flux.load_scene(os.path.join(SCENES, "demo2.yml")), flux.load_scene(DISK_SCENE)
    assert b.camera_settings == a.camera_settings and b.camera_data == a.camera_data and b.output_settings == a.output_settings
    assert b.background == a.background and len(a.shapes) == len(b.shapes)
    for i, (x, y) in enumerate(zip(a.shapes, b.shapes)):
        if i == 1:
            assert isinstance(x, flux.SphereData) and x.center == y.center and x.radius == y.radius and x.material == y.material
        else:
            assert x == y


def _doc():
    with open(DISK_SCENE) as f:
        return yaml.safe_load(f)


@pytest.mark.parametrize("radius,msg", [(None, "shapes[1].Disk: missing field `radius`"), ("five", "shapes[1].Disk.radius"),
                                        ([5.0], "shapes[1].Disk.radius"), (True, "shapes[1].Disk.radius"),
                                        (-1.0, "shapes[1].Disk.radius"), (float("nan"), "shapes[1].Disk.radius"),
                                        (float("inf"), "shapes[1].Disk.radius")])
def test_bad_radius_is_a_scene_error(flux, radius, msg):
    d = _doc()
    body = d["shapes"][1]["Disk"]
    if radius is None:
        del body["radius"]
    else:
        body["radius"] = radius
    with pytest.raises(flux.SceneError) as e:
        flux.scene_from_dict(d)
    assert msg in str(e.value)


def test_zero_radius_and_missing_fields(flux):
    d = _doc()
    d["shapes"][1]["Disk"]["radius"] = 0
    assert flux.scene_from_dict(d).shapes[1].radius == 0.0  # a degenerate disk is valid
    for key in ("center", "normal", "material"):
        d = _doc()
        del d["shapes"][1]["Disk"][key]
        with pytest.raises(flux.SceneError, match=re.escape(f"shapes[1].Disk: missing field `{key}`")):
            flux.scene_from_dict(d)
    d = _doc()
    d["shapes"][1] = {"Quad": d["shapes"][1]["Disk"]}
    with pytest.raises(flux.SceneError, match="unknown variant `Quad`.*`Disk`"):
        flux.scene_from_dict(d)


def test_shape_disk_constant_agrees_everywhere(flux):
    hdr = open(os.path.join(ROOT, "include", "flux_abi.h")).read()
    assert int(re.search(r"#define FLUX_SHAPE_DISK (\d+)", hdr).group(1)) == flux._lib.SHAPE_DISK == 2
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert int(re.search(r"pub const FLUX_SHAPE_DISK: i32 = (\d+);", md).group(1)) == 2
    assert int(re.search(r"#define FLUX_ABI_VERSION (\d+)", hdr).group(1)) == 3  # no version bump: kind 2 is the probe


def test_oracle_refuses_a_disk(flux, oracle_mod):
    """The frozen checker knows Sphere and Plane only and reads `point` from anything else: a DiskData (field `center`)
    makes it raise instead of silently rendering an infinite plane."""
    sd = flux.load_scene(DISK_SCENE)
    with pytest.raises(AttributeError):
        oracle_mod.Oracle(sd, flux.JobConfiguration(1, 2, 50), seed=1)


def test_abi_validates_the_radius_before_the_device(flux):
    """flux_ctx_create: a radius that is negative or not finite is FLUX_E_INVALID, whatever the machine; a valid disk passes
    validation (then renders, or -- on a machine without a GPU -- fails with FLUX_E_DEVICE, never FLUX_E_INVALID)."""
    base = flux.load_scene(DISK_SCENE)
    base.output_settings.image_width, base.output_settings.image_height = 8, 6
    cfg = flux.JobConfiguration(1, 2, 50)
    for bad in (-1.0, math.nan, math.inf, -math.inf):
        sd = copy.deepcopy(base)
        sd.shapes[1].radius = bad
        with pytest.raises(flux.FluxError) as e:
            flux.Renderer(sd, cfg)
        assert e.value.code == flux._lib.E_INVALID and "disk radius" in str(e.value)
    for ok in (0.0, 5.0):
        sd = copy.deepcopy(base)
        sd.shapes[1].radius = ok
        try:
            flux.Renderer(sd, cfg).close()
        except flux.FluxError as e:
            assert e.code == flux._lib.E_DEVICE, str(e)
