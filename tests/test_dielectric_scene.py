"""Dielectric materials (extension: Fresnel-sampled glass, include/flux_abi.h FLUX_MAT_DIELECTRIC) on the CPU: the Python and C++
loaders agree on scenes/glass.yml down to the flux_material bits, both reject a bad refraction index with the field's path, the node
protocol carries the material, the constant agrees across the header, the ctypes mirror and INTEGRATION.md, the C ABI validates the
index before it looks for a device, and the numpy statement of the spec (tests/dielectric_spec.py) passes its own checks."""
import copy
import math
import os
import re

import numpy as np
import pytest
import yaml

import selftest as st
from conftest import ROOT, SCENES
from extension_checks import cpp_shapes, shape_fields
from dielectric_spec import bounce, fresnel, fresnel_cos

GLASS_SCENE = os.path.join(SCENES, "glass.yml")


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    """tests/dielectric_host_selftest.cpp built against the C++ host layer (CPU only: no compute call)."""
    exe = st.build(str(tmp_path_factory.mktemp("dielectric") / "dielectric_host_selftest"), "dielectric_host_selftest.cpp", host=True, compiler="g++")
    return st.run(exe, SCENES)


def test_cpp_selftest(selftest):
    for name in ("abi scene", "yaml refraction index", "cbor round trip"):
        assert f"ok {name}" in selftest
    assert "all ok" in selftest


def test_both_loaders_give_the_same_flux_shapes(flux, selftest):
    from flux_amd.scene import SceneDesc
    sd = flux.load_scene(GLASS_SCENE)
    desc = SceneDesc(sd)
    assert desc.desc.num_shapes == 13
    assert [i for i in range(13) if desc.shapes[i].material.kind == flux._lib.MAT_DIELECTRIC] == [3, 5, 7]
    assert desc.shapes[5].material.k == 1.33 and tuple(desc.shapes[5].material.color) == (0.8, 0.95, 1.0)
    cpp = cpp_shapes(selftest)
    assert sorted(cpp) == list(range(13))
    for i in range(13):
        py = shape_fields(desc.shapes[i])
        assert py == cpp[i], (i, py, cpp[i])  # %.17g round-trips every double exactly


def test_glass_is_demo2_with_three_spheres_of_glass(flux):
    a, b = flux.load_scene(os.path.join(SCENES, "demo2.yml")), flux.load_scene(GLASS_SCENE)
    assert b.camera_settings == a.camera_settings and b.camera_data == a.camera_data and b.output_settings == a.output_settings
    assert b.background == a.background and len(a.shapes) == len(b.shapes)
    glass = {3: (1.5, (1.0, 1.0, 1.0)), 5: (1.33, (0.8, 0.95, 1.0)), 7: (1.5, (1.0, 1.0, 1.0))}
    for i, (x, y) in enumerate(zip(a.shapes, b.shapes)):
        if i in glass:
            assert isinstance(y.material, flux.DielectricData) and (y.material.refraction_index, y.material.transmit_color) == glass[i]
            assert (x.center, x.radius, x.invert) == (y.center, y.radius, y.invert)
        else:
            assert x == y


def _doc():
    with open(GLASS_SCENE) as f:
        return yaml.safe_load(f)


@pytest.mark.parametrize("ri,msg", [(None, "shapes[3].Sphere.material.Dielectric: missing field `refraction_index`"),
                                    ("glass", "shapes[3].Sphere.material.Dielectric.refraction_index"),
                                    ([1.5], "shapes[3].Sphere.material.Dielectric.refraction_index"),
                                    (True, "shapes[3].Sphere.material.Dielectric.refraction_index"),
                                    (0.0, "shapes[3].Sphere.material.Dielectric.refraction_index"),
                                    (-1.5, "shapes[3].Sphere.material.Dielectric.refraction_index"),
                                    (float("nan"), "shapes[3].Sphere.material.Dielectric.refraction_index"),
                                    (float("inf"), "shapes[3].Sphere.material.Dielectric.refraction_index")])
def test_bad_refraction_index_is_a_scene_error(flux, ri, msg):
    d = _doc()
    body = d["shapes"][3]["Sphere"]["material"]["Dielectric"]
    if ri is None:
        del body["refraction_index"]
    else:
        body["refraction_index"] = ri
    with pytest.raises(flux.SceneError) as e:
        flux.scene_from_dict(d)
    assert msg in str(e.value)


def test_missing_transmit_color_and_unknown_variant(flux):
    d = _doc()
    del d["shapes"][3]["Sphere"]["material"]["Dielectric"]["transmit_color"]
    with pytest.raises(flux.SceneError, match=re.escape("shapes[3].Sphere.material.Dielectric: missing field `transmit_color`")):
        flux.scene_from_dict(d)
    d = _doc()
    d["shapes"][3]["Sphere"]["material"] = {"Glass": d["shapes"][3]["Sphere"]["material"]["Dielectric"]}
    with pytest.raises(flux.SceneError, match="unknown variant `Glass`.*`Dielectric`"):
        flux.scene_from_dict(d)


def test_mesh_and_disk_take_the_material(flux):
    d = _doc()
    glass = {"Dielectric": {"refraction_index": 1.33, "transmit_color": [1, 1, 1]}}
    d["shapes"].append({"Disk": {"center": [0, 3, 0], "normal": [0, 1, 0], "radius": 1.0, "material": glass}})
    d["shapes"].append({"Triangle": {"v0": [0, 0, 0], "v1": [1, 0, 0], "v2": [0, 1, 0], "material": glass}})
    sd = flux.scene_from_dict(d)
    assert isinstance(sd.shapes[13].material, flux.DielectricData)
    assert isinstance(sd.shapes[14].material, flux.DielectricData)
    m = flux.scene.material_to_abi(sd.shapes[14].material)
    assert (m.kind, m.k, tuple(m.color)) == (flux._lib.MAT_DIELECTRIC, 1.33, (1.0, 1.0, 1.0))


def test_material_dielectric_constant_agrees_everywhere(flux):
    hdr = open(os.path.join(ROOT, "include", "flux_abi.h")).read()
    assert int(re.search(r"#define FLUX_MAT_DIELECTRIC (\d+)", hdr).group(1)) == flux._lib.MAT_DIELECTRIC == 4
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert int(re.search(r"pub const FLUX_MAT_DIELECTRIC: i32 = (\d+);", md).group(1)) == 4
    assert int(re.search(r"#define FLUX_ABI_VERSION (\d+)", hdr).group(1)) == 3  # no version bump: kind 4 is the probe
    from flux_amd.render import STAT_NAMES
    assert STAT_NAMES[10:] == ("dielectric_reflections", "dielectric_transmissions") and len(STAT_NAMES) <= flux._lib.NUM_STATS


def test_abi_validates_the_refraction_index_before_the_device(flux):
    """flux_ctx_create: a refraction index that is not finite or <= 0 is FLUX_E_INVALID, whatever the machine, on a shape as on a
    mesh; a valid one passes validation (then renders, or -- on a machine without a GPU -- fails with FLUX_E_DEVICE)."""
    from flux_amd.scene import MeshData
    base = flux.load_scene(GLASS_SCENE)
    base.output_settings.image_width, base.output_settings.image_height = 8, 6
    cfg = flux.JobConfiguration(1, 2, 50)
    tri = MeshData(np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), np.array([[0, 1, 2]], dtype=np.uint32),
                   flux.DielectricData(1.5, (1.0, 1.0, 1.0)))
    for where in ("shape", "mesh"):
        for bad in (0.0, -1.5, math.nan, math.inf, -math.inf):
            sd = copy.deepcopy(base)
            if where == "shape":
                sd.shapes[3].material = flux.DielectricData(bad, (1.0, 1.0, 1.0))
            else:
                sd.shapes.append(MeshData(tri.vertices, tri.triangles, flux.DielectricData(bad, (1.0, 1.0, 1.0))))
            with pytest.raises(flux.FluxError) as e:
                flux.Renderer(sd, cfg)
            assert e.value.code == flux._lib.E_INVALID and "refraction index" in str(e.value) and where in str(e.value)
    for ok in (1.0, 1.5, 0.5):
        sd = copy.deepcopy(base)
        sd.shapes[3].material = flux.DielectricData(ok, (1.0, 1.0, 1.0))
        sd.shapes.append(tri)
        try:
            flux.Renderer(sd, cfg).close()
        except flux.FluxError as e:
            assert e.code == flux._lib.E_DEVICE, str(e)


# ---- the numpy spec's self-checks ---------------------------------------------------------------------------------------

def _rays(rng, k):
    n = rng.normal(size=(k, 3)) * rng.uniform(0.3, 3.0, size=(k, 1))  # not unit: the spec normalises
    d = rng.normal(size=(k, 3)) * rng.uniform(0.3, 3.0, size=(k, 1))
    return n, d


@pytest.mark.parametrize("ri", [1.5, 1.33, 2.4, 0.7])
def test_normal_incidence(ri):
    n = np.array([[0.0, 0.0, 2.0], [0.0, 0.0, 2.0]])
    d = np.array([[0.0, 0.0, -3.0], [0.0, 0.0, 3.0]])  # from the outside, then from the inside
    F, *_ = fresnel(n, d, ri)
    want = ((ri - 1.0) / (ri + 1.0)) ** 2
    assert np.allclose(F, want, rtol=1e-14, atol=0)
    assert abs(fresnel_cos(1.0, ri) - want) < 1e-15


@pytest.mark.parametrize("ri", [1.5, 1.33, 2.4])
def test_critical_angle(ri):
    """From the inside F = 1 exactly beyond the critical angle and F < 1 before it; from the outside never 1 (but at grazing)."""
    crit = math.asin(1.0 / ri)
    th = np.concatenate([np.linspace(0.0, crit * (1 - 1e-9), 500), np.linspace(crit * (1 + 1e-9), math.pi / 2 * (1 - 1e-9), 500)])
    n = np.tile([0.0, 1.0, 0.0], (len(th), 1))
    d_in = np.column_stack([np.sin(th), np.cos(th), np.zeros_like(th)])  # inside: travelling along the normal
    F_in, *_ = fresnel(n, d_in, ri)
    before = th < crit
    assert np.all(F_in[~before] == 1.0) and np.all(F_in[before] < 1.0)
    F_out, *_ = fresnel(n, -d_in, ri)
    assert np.all(F_out < 1.0) and np.all(np.diff(F_out[before]) >= -1e-15)  # rises with the angle
    # Stokes: at the inside angle and its refracted outside angle the reflectance is the same
    sel = before & (th > 0) & (th < 0.999 * crit)  # (near the critical angle cos(t_out) is ill-conditioned)
    t_out = np.arcsin(ri * np.sin(th[sel]))
    assert np.allclose(fresnel_cos(np.cos(t_out), ri), F_in[sel], rtol=0, atol=1e-10)


def test_directions_are_unit_and_snell_holds():
    rng = np.random.default_rng(5)
    k = 20000
    for ri in (1.5, 1.33, 0.6):
        n, d = _rays(rng, k)
        u0 = np.zeros(k)  # u = 0 <= F: always reflect
        u1 = np.ones(k)  # u = 1 > F: transmit wherever there is no total internal reflection (F = 1)
        refl, wr, F = bounce(n, d, ri, u0)
        assert np.all(refl)
        assert np.allclose(np.linalg.norm(wr, axis=1), 1.0, rtol=0, atol=1e-14)
        tref, wt, _ = bounce(n, d, ri, u1)
        assert np.array_equal(tref, F == 1.0) and (~tref).sum() > k // 2
        t = ~tref
        assert np.allclose(np.linalg.norm(wt[t], axis=1), 1.0, rtol=0, atol=1e-14)
        nh = n / np.linalg.norm(n, axis=1)[:, None]
        dh = d / np.linalg.norm(d, axis=1)[:, None]
        ci = np.einsum("ij,ij->i", dh, nh)
        co = np.einsum("ij,ij->i", wt, nh)
        # the reflection keeps the side of the incoming ray, the transmission crosses the surface
        assert np.all(np.einsum("ij,ij->i", wr, nh) * ci < 0) and np.all(co[t] * ci[t] > 0)
        # Snell: eta1 sin(theta_i) = eta2 sin(theta_t), the index `ri` on the side the normal points away from
        sin_i = np.linalg.norm(np.cross(dh, nh), axis=1)
        sin_t = np.linalg.norm(np.cross(wt, nh), axis=1)
        outside = ci < 0
        lhs = np.where(outside, 1.0 * sin_i, ri * sin_i)
        rhs = np.where(outside, ri * sin_t, 1.0 * sin_t)
        assert np.allclose(lhs[t], rhs[t], rtol=0, atol=1e-13)
        # the three vectors are coplanar
        assert np.allclose(np.einsum("ij,ij->i", np.cross(dh, nh), wt)[t], 0.0, atol=1e-13)


def test_energy_split():
    """With u uniform on (0, 1] the reflected share is F: the stratified u of one depth row decide as the spec says."""
    n = np.tile([0.0, 0.0, 1.0], (4096, 1))
    d = np.tile([0.6, 0.0, -0.8], (4096, 1))
    u = 1.0 - (np.arange(4096) + 0.5) / 4096
    refl, _, F = bounce(n, d, 1.5, u)
    assert abs(refl.mean() - F[0]) <= 1.0 / 4096
