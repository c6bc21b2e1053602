"""Disk shapes (extension, include/flux_abi.h FLUX_SHAPE_DISK) on the device, in every render kernel.

The CPU checker is frozen and knows no disk, so the evidence comes three ways:
  1. plane equivalence: a disk of radius 1e3 in place of demo1's / demo2's plane holds every hit nearer than their r = 100
     environment sphere, so the frames (and the path statistics) must be the plane scene's -- which the oracle checks;
  2. rays: Scene::hit / Scene::shade of random rays (flux_debug_shade) against numpy's evaluation of the spec;
  3. a closed form: a Matte floor under an emissive disk.
"""
import copy
import math
import os

import numpy as np
import pytest

from conftest import SCENES, small_scene
from extension_checks import cli_frame, host_bins, loopback_frames, math_mode, node_frame, render, set_sharded_frame, small_yaml

pytestmark = pytest.mark.gpu

T_MIN = 0.0005


def _plane_to_disk(flux, sd, radius=1e3):
    s = copy.deepcopy(sd)
    for i, sh in enumerate(s.shapes):
        if isinstance(sh, flux.PlaneData):
            s.shapes[i] = flux.DiskData(sh.point, sh.normal, radius, sh.material)
    return s


def _small_mesh(flux):
    """Two Matte triangles standing on the floor between demo2's spheres (BVH kernels)."""
    from flux_amd.scene import MeshData
    v = np.array([[-3.0, 0.0, 1.0], [0.5, 0.0, 3.0], [0.5, 2.5, 3.0], [-3.0, 2.5, 1.0]])
    t = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint32)
    return MeshData(v, t, flux.MatteData((0.6, 0.8, 0.5), (0, 0, 0), 0.9))


@pytest.mark.parametrize("scene", ["demo1", "demo2"])
@pytest.mark.parametrize("math_name", ["fast", "strict"])
def test_plane_equivalence(flux, oracle_mod, demo1, demo2, scene, math_name):
    plane = small_scene(demo1 if scene == "demo1" else demo2, 64, 48)
    disk = _plane_to_disk(flux, plane)
    m = math_mode(flux, math_name)
    for n in (4, 16):
        want_o = oracle_mod.Oracle(plane, flux.JobConfiguration(n, 5, 50), seed=1)
        o_img = want_o.render_frame(threads=8) if n == 4 or scene == "demo2" else None
        o_stats = want_o.stats() if o_img is not None else None
        for kernel in (flux.KERNEL_STATIC, flux.KERNEL_REFILL, flux.KERNEL_SPLIT):
            a, sa, _ = render(flux, plane, n, m, kernel)
            b, sb, _ = render(flux, disk, n, m, kernel)
            assert sa == sb, (n, kernel, sa, sb)
            assert np.abs(a - b).max() <= 1e-12, (n, kernel)
            assert np.array_equal(a, b), (n, kernel)  # bit-equal: the same operations decide every hit
            if o_img is not None:
                assert np.abs(b - o_img).max() < 1e-4, (n, kernel)
                assert {k: sb[k] for k in o_stats} == o_stats, (n, kernel)


@pytest.mark.parametrize("math_name", ["fast", "strict"])
def test_plane_equivalence_with_a_mesh(flux, oracle_mod, demo2, math_name):
    plane = small_scene(demo2, 64, 48)
    plane.shapes.append(_small_mesh(flux))
    disk = _plane_to_disk(flux, plane)
    m = math_mode(flux, math_name)
    n = 8
    o = oracle_mod.Oracle(plane, flux.JobConfiguration(n, 5, 50), seed=1)
    o_img = o.render_frame(threads=8)
    o_stats = o.stats()
    plans = set()
    for traversal in (flux._lib.TRAVERSE_BVH, flux._lib.TRAVERSE_BVH_BINARY, flux._lib.TRAVERSE_BRUTE):
        a, sa, pa = render(flux, plane, n, m, traversal=traversal)
        b, sb, pb = render(flux, disk, n, m, traversal=traversal)
        plans.add(pb["kernel"])
        assert pa["kernel"] == pb["kernel"]
        assert sa == sb, (traversal, sa, sb)
        assert np.array_equal(a, b), traversal
        assert np.abs(b - o_img).max() < 1e-4, traversal
        assert {k: sb[k] for k in o_stats if k not in ("bvh_nodes", "tris_tested")} == \
            {k: v for k, v in o_stats.items() if k not in ("bvh_nodes", "tris_tested")}
    if math_name == "fast":
        assert flux._lib.PLAN_BVH4 in plans and flux._lib.PLAN_BVH_BINARY in plans


@pytest.mark.parametrize("math_name", ["fast", "strict"])
def test_out_of_reach_disk_changes_nothing(flux, demo2, math_name):
    """A disk under the floor (every ray that could reach it meets the infinite floor first), listed second so that every
    later YAML index moves by one."""
    base = small_scene(demo2, 64, 48)
    far = copy.deepcopy(base)
    far.shapes.insert(1, flux.DiskData((0.0, -50.0, 3.0), (0.0, 1.0, 0.0), 10.0, flux.EmissiveData((1.0, 0.0, 0.0), 50.0)))
    m = math_mode(flux, math_name)
    for n, kernel in ((4, flux.KERNEL_STATIC), (8, flux.KERNEL_REFILL), (16, flux.KERNEL_SPLIT)):
        a, sa, _ = render(flux, base, n, m, kernel)
        b, sb, _ = render(flux, far, n, m, kernel)
        assert sa == sb and np.abs(a - b).max() <= 1e-12 and np.array_equal(a, b), (n, kernel)


# ---- rays ----------------------------------------------------------------------------------------------------------

BG = (0.1, 0.2, 0.3)
EMIT = (0.7, 0.45, 0.25)  # colour; power 2 -> L = (1.4, 0.9, 0.5)
POWER = 2.0


def _ray_scene(flux, shapes):
    return flux.SceneData("rays", flux.OutputSettings(8, 8, 1.0), BG, shapes, flux.CameraSettings((0, 0, -5), (0, 0, 0), (0, 1, 0)),
                          flux.CameraData(1.0, 100.0, 100.0, 0.0))


def _spec(o, d, c, n, rr, strict=True):
    """numpy's Disk::hit, operations in the kernels' order: (t, hit, rim) per ray."""
    num = (c[0] - o[:, 0]) * n[0] + (c[1] - o[:, 1]) * n[1] + (c[2] - o[:, 2]) * n[2]
    den = d[:, 0] * n[0] + d[:, 1] * n[1] + d[:, 2] * n[2]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = num / den
        q = o + t[:, None] * d
        e = q - np.asarray(c)
        r2 = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2]
        hit = (t > T_MIN) & (r2 <= rr)
        rim = np.abs(r2 - rr) <= 1e-9 * max(rr, 1e-300)
    return t, hit, rim


def _expected_rgb(d, n, hit):
    front = ((n[0] * -1.0) * d[:, 0] + (n[1] * -1.0) * d[:, 1] + (n[2] * -1.0) * d[:, 2]) > 0.0
    L = np.array(EMIT) * POWER
    rgb = np.tile(np.array(BG), (len(d), 1))
    rgb[hit & front] = L
    rgb[hit & ~front] = 0.0
    return rgb, front


def _random_rays(rng, c, n, radius, count):
    o = rng.uniform(-4, 4, size=(count, 3))
    # half aimed at points of the disk's plane near the disk (in and out of it), half in random directions
    a = np.cross(n, [0.3, 1.0, 0.7])
    a /= np.linalg.norm(a)
    b = np.cross(n, a)
    b /= np.linalg.norm(b)
    rad = radius * 1.6 * np.sqrt(rng.uniform(0, 1, count))
    ph = rng.uniform(0, 2 * np.pi, count)
    target = np.asarray(c) + (rad * np.cos(ph))[:, None] * a + (rad * np.sin(ph))[:, None] * b
    d = target - o
    k = count // 2
    d[k:] = rng.normal(size=(count - k, 3))
    d *= rng.uniform(0.5, 2.0, size=(count, 1))  # not unit vectors: the spec takes d as given
    return o, d


@pytest.mark.parametrize("math_name", ["fast", "strict"])
def test_random_rays_against_the_spec(flux, math_name):
    rng = np.random.default_rng(7)
    c = (0.4, 1.3, -0.2)
    n = np.array([0.3, -1.2, 0.5])
    n = tuple(n / np.linalg.norm(n))
    radius = 1.7
    sd = _ray_scene(flux, [flux.DiskData(c, n, radius, flux.EmissiveData(EMIT, POWER))])
    o, d = _random_rays(rng, c, n, radius, 100000)
    with flux.Renderer(sd, flux.JobConfiguration(2, 3, 50), seed=2) as r:
        r.set_math(math_mode(flux, math_name))
        rgb, hit, t = r.debug_shade(o, d, 1, 0, 0)
    tw, hw, rim = _spec(o, d, c, n, radius * radius)
    keep = ~rim
    assert keep.sum() > 99000 and hw[keep].sum() > 20000
    assert np.array_equal(hit[keep] == 0, hw[keep]) and np.all((hit == 0) | (hit == -1))
    h = keep & hw
    if math_name == "strict":
        assert np.array_equal(t[h], tw[h])
    else:
        assert np.allclose(t[h], tw[h], rtol=1e-11, atol=0)  # FAST fuses the operations of t into FMAs
    want, front = _expected_rgb(d, n, hw)
    assert np.array_equal(rgb[keep], want[keep])
    assert (h & front).sum() > 5000 and (h & ~front).sum() > 5000


@pytest.mark.parametrize("math_name", ["fast", "strict"])
def test_ray_corner_cases(flux, math_name):
    m = math_mode(flux, math_name)
    cfg = flux.JobConfiguration(2, 3, 50)
    emis = flux.EmissiveData(EMIT, POWER)
    c = (0.0, 2.0, 0.0)
    down = (0.0, -1.0, 0.0)
    # parallel rays (d.n == 0 exactly): in the disk's plane (t = 0/0) and beside it (t = +-inf) -- never a hit
    o = np.array([[0.5, 2.0, 0.0], [0.0, 2.0, 0.3], [0.5, 2.5, 0.0], [0.0, 1.0, 0.0]])
    d = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.3], [0.2, 0.0, 1.0]])
    # rays starting on the disk (t = 0 <= T_MIN), and a hit just past T_MIN
    o2 = np.array([[0.3, 2.0, 0.1], [0.0, 2.0 - 0.4 * T_MIN, 0.0], [0.0, 2.0 - 4 * T_MIN, 0.0]])
    d2 = np.array([[0.0, 1.0, 0.0], [0.0, 1.0, 0.0], [0.0, 1.0, 0.0]])
    sd = _ray_scene(flux, [flux.DiskData(c, down, 1.0, emis)])
    with flux.Renderer(sd, cfg) as r:
        r.set_math(m)
        rgb, hit, t = r.debug_shade(np.vstack([o, o2]), np.vstack([d, d2]), 1, 0, 0)
    assert list(hit) == [-1, -1, -1, -1, -1, -1, 0]
    assert np.array_equal(rgb[:6], np.tile(BG, (6, 1))) and np.array_equal(rgb[6], np.array(EMIT) * POWER)
    rng = np.random.default_rng(3)
    o3, d3 = _random_rays(rng, c, np.array(down), 1.0, 4000)
    # zero radius and zero normal: random rays never hit; a ray aimed at the zero-radius disk's centre hits iff the spec says so
    for shape in (flux.DiskData(c, down, 0.0, emis), flux.DiskData(c, (0.0, 0.0, 0.0), 1.0, emis)):
        with flux.Renderer(_ray_scene(flux, [shape]), cfg) as r:
            r.set_math(m)
            rgb, hit, t = r.debug_shade(o3, d3, 1, 0, 0)
        assert np.all(hit == -1) and np.array_equal(rgb, np.tile(BG, (len(o3), 1)))
    if math_name == "strict":
        oc = np.array([[0.0, 0.0, 0.0], [0.25, 0.5, -0.75]])
        dc = np.asarray(c) - oc
        _, hw, _ = _spec(oc, dc, c, down, 0.0)
        with flux.Renderer(_ray_scene(flux, [flux.DiskData(c, down, 0.0, emis)]), cfg) as r:
            r.set_math(m)
            _, hit, _ = r.debug_shade(oc, dc, 1, 0, 0)
        assert np.array_equal(hit == 0, hw)


@pytest.mark.parametrize("math_name", ["fast", "strict"])
def test_tie_with_a_coplanar_plane(flux, math_name):
    """Equal t: the lower YAML index wins, whichever of the two is scanned first (planes are scanned before disks)."""
    m = math_mode(flux, math_name)
    c, up = (0.2, 0.5, -0.1), (0.0, 1.0, 0.0)
    emis = flux.EmissiveData(EMIT, POWER)
    matte = flux.MatteData((0.5, 0.5, 0.5), (0, 0, 0), 1.0)
    rng = np.random.default_rng(11)
    o = np.column_stack([rng.uniform(-1, 1, 2000), rng.uniform(1.0, 3.0, 2000), rng.uniform(-1, 1, 2000)])
    d = np.column_stack([rng.uniform(-0.3, 0.3, 2000), -np.ones(2000), rng.uniform(-0.3, 0.3, 2000)])
    _, inside, rim = _spec(o, d, c, up, 0.8 ** 2)
    keep = ~rim
    assert inside[keep].sum() > 500 and (~inside[keep]).sum() > 100
    cfg = flux.JobConfiguration(2, 3, 50)
    for first in ("disk", "plane"):
        disk, plane = flux.DiskData(c, up, 0.8, emis), flux.PlaneData(c, up, matte)
        shapes = [disk, plane] if first == "disk" else [plane, disk]
        with flux.Renderer(_ray_scene(flux, shapes), cfg) as r:
            r.set_math(m)
            _, hit, _ = r.debug_shade(o, d, 1, 0, 0)
        di, pi = (0, 1) if first == "disk" else (1, 0)
        if first == "disk":
            assert np.all(hit[keep & inside] == di) and np.all(hit[keep & ~inside] == pi)
        else:
            assert np.all(hit[keep] == pi)


# ---- closed form ------------------------------------------------------------------------------------------------------

def _solid_angle(x, z, a, h, nr=96, nphi=192):
    """Solid angle of the disk (radius a, centre (0, h, 0), parallel to the floor) seen from floor points (x, 0, z):
    Omega = int h / R^3 dA, Gauss-Legendre in r, the midpoint rule in phi (periodic: spectrally accurate)."""
    gr, wr = np.polynomial.legendre.leggauss(nr)
    r = 0.5 * a * (gr + 1.0)
    wr = 0.5 * a * wr
    phi = (np.arange(nphi) + 0.5) * 2 * np.pi / nphi
    px = (r[:, None] * np.cos(phi)[None, :]).ravel()
    pz = (r[:, None] * np.sin(phi)[None, :]).ravel()
    w = ((wr * r)[:, None] * np.full(nphi, 2 * np.pi / nphi)[None, :]).ravel()
    dx = x.ravel()[:, None] - px[None, :]
    dz = z.ravel()[:, None] - pz[None, :]
    R2 = dx * dx + dz * dz + h * h
    return (h / (R2 * np.sqrt(R2)) @ w).reshape(x.shape)


def _floor_scene(flux, a, h, normal_y, W=32):
    eye_h, vpd = 1.0, 100.0
    ps = 1.5 * vpd / (W / 2 * eye_h)  # the image spans |x|, |z| <= 1.5 on the floor
    shapes = [flux.PlaneData((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), flux.MatteData((0.5, 1.0, 0.75), (0, 0, 0), 0.9)),
              flux.DiskData((0.0, h, 0.0), (0.0, normal_y, 0.0), a, flux.EmissiveData((0.9, 0.6, 0.3), 1.0))]
    sd = flux.SceneData("floor", flux.OutputSettings(W, W, ps), (0.0, 0.0, 0.0), shapes,
                        flux.CameraSettings((0.0, eye_h, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0)), flux.CameraData(1.0, vpd, vpd, 0.0))
    return sd, eye_h, vpd, ps


@pytest.mark.parametrize("math_name", ["fast", "strict"])
def test_closed_form_floor_under_a_disk(flux, math_name):
    a, h, W, n = 1.0, 2.0, 32, 64
    rho = np.array([0.5, 1.0, 0.75]) * 0.9
    L = np.array([0.9, 0.6, 0.3])
    assert (rho * L).max() < 1.0  # max_to_one never clamps a sample
    # on the axis: p = Omega / 2 pi = 1 - h / sqrt(h^2 + a^2)
    assert abs(_solid_angle(np.zeros(1), np.zeros(1), a, h)[0] / (2 * np.pi) - (1 - h / math.hypot(h, a))) < 1e-12
    sd, eye_h, vpd, ps = _floor_scene(flux, a, h, -1.0, W)
    with flux.Renderer(sd, flux.JobConfiguration(n, 2, 50), seed=5) as r:
        r.set_math(math_mode(flux, math_name))
        img = r.render_frame()
    # pixel (row, col) sees the floor at (e/d) (u U + v V), u = aps (col - W/2 + sx), v = aps ((H - row) - H/2 + sy), U = -x, V = +z:
    # Omega averaged over the footprint (4 x 4 points per pixel)
    s = (np.arange(4) + 0.5) / 4
    cols = (np.arange(W)[:, None] - W / 2 + s[None, :]).ravel()
    rows = ((W - np.arange(W))[:, None] - W / 2 + s[None, :]).ravel()
    zz, xx = np.meshgrid(rows * ps * eye_h / vpd, -cols * ps * eye_h / vpd, indexing="ij")
    p = (_solid_angle(xx, zz, a, h) / (2 * np.pi)).reshape(W, 4, W, 4).mean(axis=(1, 3))
    want = p[:, :, None] * (rho * L)[None, None, :]
    spp = n * n
    sigma = (rho * L)[None, None, :] * np.sqrt(p * (1 - p) / spp)[:, :, None]
    assert np.all(np.abs(img - want) <= 5 * sigma + 1e-12), np.abs((img - want) / sigma).max()
    patch = slice(W // 2 - 4, W // 2 + 4)
    err = np.abs(img[patch, patch].mean(axis=(0, 1)) - want[patch, patch].mean(axis=(0, 1)))
    assert np.all(err <= 5 * sigma[patch, patch].mean(axis=(0, 1)) / 8), err
    # flipped: the disk faces away from the floor, which then receives nothing at all
    sd2, *_ = _floor_scene(flux, a, h, 1.0, W)
    with flux.Renderer(sd2, flux.JobConfiguration(8, 2, 50), seed=5) as r:
        r.set_math(math_mode(flux, math_name))
        assert np.all(r.render_frame() == 0.0)


# ---- plumbing ---------------------------------------------------------------------------------------------------------

def _disk_light(flux, w=64, h=48):
    return small_scene(flux.load_scene(os.path.join(SCENES, "disk_light.yml")), w, h)


def test_set_shares_and_loopback_ranks(flux):
    sd = _disk_light(flux, 50, 37)
    cfg = flux.JobConfiguration(8, 5, 50)
    with flux.Renderer(sd, cfg, seed=11) as r:
        want = r.render_frame()
        for world in (1, 2, 3):
            assert np.array_equal(set_sharded_frame(flux, r, world).numpy(), want), world
    for G, _, frame in loopback_frames(flux, sd, cfg, 11, (2, 3), (flux.SHARD_SETS,)):
        assert np.array_equal(frame, want), G


def test_cli_and_node_write_the_python_frame(flux, tmp_path):
    flux_bin, node_bin = host_bins()
    scene = small_yaml(os.path.join(SCENES, "disk_light.yml"), tmp_path, 64, 48)
    sd = flux.load_scene(scene)
    assert sd.output_settings.image_width == 64 and isinstance(sd.shapes[1], flux.DiskData)
    with flux.Renderer(sd, flux.JobConfiguration(3, 5, 16), seed=5) as r:
        want_img = r.render_frame()
    flux.write_ppm(str(tmp_path / "want.ppm"), want_img)
    want = open(tmp_path / "want.ppm", "rb").read()
    common = ["-r", "3", "-d", "5", "-R", "16", "--seed", "5"]
    assert cli_frame(flux_bin, scene, common, tmp_path / "direct") == want
    assert node_frame(flux_bin, node_bin, scene, common, tmp_path / "remote", tmp_path) == want


def test_launch_plans(flux):
    sd = flux.load_scene(os.path.join(SCENES, "disk_light.yml"))
    with flux.Renderer(sd, flux.JobConfiguration(16, 5, 50), seed=1) as r:
        assert r.launch_plan()["kernel"] == flux._lib.PLAN_SPLIT
    # disks whose hit records overflow the split kernel's 16 KiB of LDS: the refill kernel, as for too many spheres
    many = _disk_light(flux, 16, 12)
    for k in range(200):
        many.shapes.append(flux.DiskData((0.1 * k, -30.0, 0.0), (0.0, 1.0, 0.0), 0.01, many.shapes[-1].material))
    with flux.Renderer(many, flux.JobConfiguration(16, 5, 50), seed=1) as r:
        assert r.launch_plan()["kernel"] == flux._lib.PLAN_REFILL
        img = r.render_frame()
    with flux.Renderer(_disk_light(flux, 16, 12), flux.JobConfiguration(16, 5, 50), seed=1) as r:
        r.set_kernel(flux.KERNEL_REFILL)
        assert np.array_equal(r.render_frame(), img)  # disks under the floor are out of reach
