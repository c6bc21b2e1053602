"""Dielectric materials (extension, include/flux_abi.h FLUX_MAT_DIELECTRIC) on the device, in every render kernel.

The CPU checker is frozen and knows no glass, so the evidence comes from the spec stated in numpy (tests/dielectric_spec.py),
closed forms and agreement between kernels:
  1. rays: Scene::shade of random rays (flux_debug_shade) through a glass plane, disk, sphere and two-triangle mesh between two
     distinctly coloured emitters, against numpy's path for each ray (u from the context's own hemi table);
  2. the Fresnel closed form of a glass plane under an emissive sky, seen through a pinhole;
  3. a white furnace: every sample is 1 or lost to the depth limit;
  4. the kernels agree with each other; 5. shares and loopback ranks; 6. index 1 changes nothing; 7. the CLI writes the frame.
"""
import copy
import os

import numpy as np
import pytest

from conftest import SCENES, small_scene
from dielectric_spec import bounce, fresnel_cos
from switches import switches  # noqa: F401 (the fixture)
from extension_checks import cli_frame, host_bins, loopback_frames, math_mode, render, row_tiles, set_sharded_frame, small_yaml

pytestmark = pytest.mark.gpu

T_MIN = 0.0005


def _glass(small=(64, 48)):
    import flux_amd as flux
    return small_scene(flux.load_scene(os.path.join(SCENES, "glass.yml")), *small)


# ---- 1. rays against the spec --------------------------------------------------------------------------------------

BG = (0.0, 0.0, 0.0)
TOP = (1.0, 0.5, 0.25)      # the emitter on the normal's side
BOTTOM = (0.125, 0.75, 1.0)  # the emitter on the other side
TC = (0.5, 0.875, 0.75)      # transmit_color
RI = 1.5
DEPTH = 12


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


class _Target:
    """One glass target and numpy's intersection with it: (t, normal) per ray, t = inf where it misses."""

    def __init__(self, kind, nt):
        self.kind, self.nt = kind, _unit(nt)
        a = np.cross(self.nt, [0.3, 1.0, 0.7])
        self.a = a / np.linalg.norm(a)
        self.b = np.cross(self.nt, self.a)

    def shapes(self, flux, mat):
        from flux_amd.scene import MeshData
        if self.kind == "plane":
            return [flux.PlaneData((0.0, 0.0, 0.0), tuple(self.nt), mat)]
        if self.kind == "disk":
            return [flux.DiskData((0.0, 0.0, 0.0), tuple(2.5 * self.nt), 2.0, mat)]  # a non-unit normal: the spec normalises it
        if self.kind == "sphere":
            return [flux.SphereData((0.0, 0.0, 0.0), 1.5, mat, False)]
        q = np.array([-2 * self.a - 2 * self.b, 2 * self.a - 2 * self.b, 2 * self.a + 2 * self.b, -2 * self.a + 2 * self.b])
        return [MeshData(q, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint32), mat)]

    def normal(self):  # the stored normal of the planar targets (the mesh: normalize(e1 x e2) of its triangles, = nt by winding)
        return 2.5 * self.nt if self.kind == "disk" else self.nt

    def hit(self, o, d):
        if self.kind == "sphere":
            b = np.einsum("ij,ij->i", o, d)
            a = np.einsum("ij,ij->i", d, d)
            c = np.einsum("ij,ij->i", o, o) - 1.5 * 1.5
            disc = b * b - a * c
            with np.errstate(invalid="ignore"):
                e = np.sqrt(disc)
                t0, t1 = (-b - e) / a, (-b + e) / a
            t = np.where(t0 > T_MIN, t0, np.where(t1 > T_MIN, t1, np.inf))
            t = np.where(disc >= 0, t, np.inf)
            n = (o + t[:, None] * d) / 1.5
            return t, n
        nt = self.nt
        with np.errstate(divide="ignore", invalid="ignore"):
            t = -(o @ nt) / (d @ nt)
        t = np.where(t > T_MIN, t, np.inf)
        q = o + np.where(np.isfinite(t), t, 0.0)[:, None] * d
        if self.kind == "disk":
            t = np.where(np.einsum("ij,ij->i", q, q) <= 4.0, t, np.inf)
        elif self.kind == "mesh":
            t = np.where((np.abs(q @ self.a) <= 2.0) & (np.abs(q @ self.b) <= 2.0), t, np.inf)
        return t, np.tile(self.normal(), (len(o), 1))


def _emitters(flux, nt):
    return [flux.PlaneData(tuple(6.0 * nt), tuple(-nt), flux.EmissiveData(TOP, 1.0)),
            flux.PlaneData(tuple(-6.0 * nt), tuple(nt), flux.EmissiveData(BOTTOM, 1.0))]


def _trace(tg, o, d, hemi_col, ri):
    """numpy's path for each ray: rgb folded as STRICT folds it, the number of bounces, and the smallest |u - F| met."""
    k = len(o)
    nt = tg.nt
    alive = np.ones(k, dtype=bool)
    L = np.zeros((k, 3))
    weights = []  # per bounce: [k, 3] (1 where the path had ended)
    margin = np.full(k, np.inf)
    nb = np.zeros(k, dtype=int)
    o, d = o.copy(), d.copy()
    for depth in range(1, DEPTH + 2):
        if depth > DEPTH:  # scene.rs:164-165: the path is lost
            L[alive] = 0.0
            break
        t, n = tg.hit(o, d)
        # the emitters: planes at +-6 nt; a ray that misses everything sees the black background
        dn = d @ nt
        with np.errstate(divide="ignore", invalid="ignore"):
            tt = (6.0 - o @ nt) / dn
            tb = (-6.0 - o @ nt) / dn
        tt = np.where(tt > T_MIN, tt, np.inf)
        tb = np.where(tb > T_MIN, tb, np.inf)
        glass = alive & (t < tt) & (t < tb)
        end_top = alive & ~glass & np.isfinite(tt)
        end_bot = alive & ~glass & ~end_top & np.isfinite(tb)
        L[end_top] = TOP
        L[end_bot] = BOTTOM
        u = hemi_col[depth - 1]
        refl, wi, F = bounce(n[glass], d[glass], ri, np.full(glass.sum(), u))
        margin[glass] = np.minimum(margin[glass], np.abs(u - F))
        w = np.ones((k, 3))
        w[np.flatnonzero(glass)[~refl]] = TC
        weights.append(w)
        nb[glass] += 1
        o[glass] = o[glass] + t[glass][:, None] * d[glass]
        d[glass] = wi
        alive = glass
        if not alive.any():
            break
    for w in reversed(weights):
        L = (w * L) * 1.0
    return L, nb, margin


def _rays(rng, tg, count):
    """Half from the normal's side, half from the other; origins low over the surface and far to the side reach total
    internal reflection from the back.  The sphere: half from outside aimed within 0.9 r of its centre, half from inside."""
    k = count // 2
    s = np.where(np.arange(count) < k, 1.0, -1.0)
    if tg.kind == "sphere":
        o = np.empty((count, 3))
        d = rng.normal(size=(count, 3))
        dirs = rng.normal(size=(k, 3))
        dirs /= np.linalg.norm(dirs, axis=1)[:, None]
        o[:k] = dirs * rng.uniform(2.0, 4.5, size=(k, 1))
        off = rng.normal(size=(k, 3))
        off -= np.einsum("ij,ij->i", off, dirs)[:, None] * dirs
        off *= (1.35 * np.sqrt(rng.uniform(0, 1, k)) / np.linalg.norm(off, axis=1))[:, None]
        d[:k] = off - o[:k]
        ins = rng.normal(size=(count - k, 3))
        o[k:] = ins / np.linalg.norm(ins, axis=1)[:, None] * (1.2 * rng.uniform(0, 1, size=(count - k, 1)) ** (1 / 3))
    else:
        lim = 1.6
        h = s * rng.uniform(0.05, 4.0, count)
        side = rng.uniform(-5.0, 5.0, size=(count, 2))
        o = h[:, None] * tg.nt + side[:, :1] * tg.a + side[:, 1:] * tg.b
        aim = rng.uniform(-lim, lim, size=(count, 2)) if tg.kind == "mesh" else \
            (lim * np.sqrt(rng.uniform(0, 1, count)))[:, None] * np.column_stack([np.cos(p := rng.uniform(0, 2 * np.pi, count)), np.sin(p)])
        q = aim[:, :1] * tg.a + aim[:, 1:] * tg.b
        d = q - o
    d *= rng.uniform(0.5, 2.0, size=(count, 1))  # not unit vectors: the spec normalises d
    return o, d


@pytest.mark.parametrize("math_name", ["fast", "strict"])
@pytest.mark.parametrize("kind", ["plane", "disk", "sphere", "mesh"])
def test_random_rays_against_the_spec(flux, kind, math_name):
    rng = np.random.default_rng({"plane": 1, "disk": 2, "sphere": 3, "mesh": 4}[kind])
    tg = _Target(kind, (0.3, 1.0, -0.4))
    shapes = tg.shapes(flux, flux.DielectricData(RI, TC))
    sd = flux.SceneData("rays", flux.OutputSettings(8, 8, 1.0), BG,
                        _emitters(flux, tg.nt) + shapes if kind == "mesh" else shapes + _emitters(flux, tg.nt),
                        flux.CameraSettings((0, 0, -5), (0, 0, 0), (0, 1, 0)), flux.CameraData(1.0, 100.0, 100.0, 0.0))
    target_ids = {2, 3} if kind == "mesh" else {0}
    per, batches = 5000, 24
    o, d = _rays(rng, tg, per * batches)
    total = {"rays": 0, "excluded": 0, "reflect": 0, "transmit": 0, "multi": 0}
    with flux.Renderer(sd, flux.JobConfiguration(8, DEPTH, 50), seed=3) as r:
        r.set_math(math_mode(flux, math_name))
        hemi = r.table(flux._lib.TABLE_HEMI)  # [set][depth][sample][xyz]
        u1 = hemi[0, 0, :, 2]
        # the samples whose first u spreads over (0, 0.7): both branches at every angle band
        picks = np.argsort(u1)[np.linspace(0, int(0.7 * len(u1)), batches).astype(int)]
        for b, smp in enumerate(picks):
            sl = slice(b * per, (b + 1) * per)
            rgb, hit, _ = r.debug_shade(o[sl], d[sl], 1, 0, int(smp))
            want, nb, margin = _trace(tg, o[sl], d[sl], hemi[0, :, smp, 2], RI)
            assert set(np.unique(hit)) <= target_ids, (b, np.unique(hit))
            keep = margin >= 1e-9
            total["rays"] += per
            total["excluded"] += int((~keep).sum())
            total["multi"] += int((keep & (nb > 1)).sum())
            if math_name == "strict":
                bad = keep & np.any(rgb != want, axis=1)
            else:
                bad = keep & np.any(np.abs(rgb - want) > 1e-12, axis=1)
            assert not bad.any(), (b, int(bad.sum()), np.flatnonzero(bad)[:5], rgb[bad][:3], want[bad][:3], nb[bad][:3])
            _, n0 = tg.hit(o[sl], d[sl])
            first = bounce(n0, d[sl], RI, np.full(per, hemi[0, 0, smp, 2]))[0]
            total["reflect"] += int((keep & first).sum())
            total["transmit"] += int((keep & ~first).sum())
    print(f"{kind} {math_name}: {total}")
    assert total["excluded"] <= total["rays"] // 1000, total
    assert total["reflect"] > 5000 and total["transmit"] > 5000, total
    if kind == "sphere":  # through the sphere and inside it: paths of several glass bounces
        assert total["multi"] > 10000, total


def test_inside_a_sphere_total_internal_reflection(flux):
    """Rays from inside a glass sphere at grazing incidence reflect totally, many times over: each segment must find the sphere
    again (the self-skip applies only to a segment that leaves a convex sphere outwards), until the depth limit ends the path."""
    tg = _Target("sphere", (0.0, 1.0, 0.0))
    sd = flux.SceneData("rays", flux.OutputSettings(8, 8, 1.0), BG, tg.shapes(flux, flux.DielectricData(RI, TC)) + _emitters(flux, tg.nt),
                        flux.CameraSettings((0, 0, -5), (0, 0, 0), (0, 1, 0)), flux.CameraData(1.0, 100.0, 100.0, 0.0))
    # start near the surface and travel almost along it: incidence ~80 degrees from the normal, beyond asin(1/1.5)
    phi = np.linspace(0, 2 * np.pi, 256, endpoint=False)
    o = np.column_stack([1.45 * np.cos(phi), 0.1 * np.sin(3 * phi), 1.45 * np.sin(phi)])
    d = np.column_stack([-np.sin(phi), 0.02 * np.cos(phi), np.cos(phi)])
    for m in ("fast", "strict"):
        with flux.Renderer(sd, flux.JobConfiguration(2, DEPTH, 50), seed=3) as r:
            r.set_math(math_mode(flux, m))
            rgb, hit, _ = r.debug_shade(o, d, 1, 0, 0)
        assert np.all(hit == 0) and np.all(rgb == 0.0), m  # lost to the depth limit: never escaped
        want, nb, _ = _trace(tg, o, d, np.ones(DEPTH), RI)
        assert np.all(nb == DEPTH) and np.all(want == 0.0)


# ---- 2. the Fresnel closed form ------------------------------------------------------------------------------------

SKY = (1.0, 0.5, 0.25)  # dyadic: sums of equal samples are exact


def _fresnel_scene(flux, normal_y, W=32, ps=2.0):
    shapes = [flux.PlaneData((0.0, 0.0, 0.0), (0.0, normal_y, 0.0), flux.DielectricData(1.5, (1.0, 1.0, 1.0))),
              flux.DiskData((0.0, 10.0, 0.0), (0.0, -1.0, 0.0), 1e4, flux.EmissiveData(SKY, 1.0))]
    return flux.SceneData("fresnel", flux.OutputSettings(W, W, ps), (0.0, 0.0, 0.0), shapes,
                          flux.CameraSettings((0.0, 3.0, 0.0), (0.0, 0.0, 6.0), (0.0, 1.0, 0.0)), flux.CameraData(1.0, 100.0, 100.0, 0.0))


def _incidence_cos(basis, W, ps, cols, rows, sx, sy):
    """cos(theta) of pixel (rows, cols) at sample offsets (sx, sy): u = aps (col - W/2 + sx), v = aps ((H - row) - H/2 + sy)."""
    U, V, Wv = basis
    u = ps * ((cols - W / 2) + sx)
    v = ps * (((W - rows) - W / 2) + sy)
    d = u[..., None] * U + v[..., None] * V - 100.0 * Wv
    d /= np.linalg.norm(d, axis=-1)[..., None]
    return -d[..., 1]  # cos(theta) against the plane's normal (0, 1, 0)


@pytest.mark.parametrize("math_name", ["fast", "strict"])
def test_fresnel_closed_form(flux, math_name):
    W, ps, root = 32, 2.0, 8
    n = root * root
    with flux.Renderer(_fresnel_scene(flux, 1.0, W, ps), flux.JobConfiguration(root, 3, 50), seed=5) as r:
        r.set_math(math_mode(flux, math_name))
        r.enable_stats(True)
        r.stats(reset=True)
        img = r.render_frame()
        st = r.stats()
        basis = r.camera_basis()
    # F over each pixel's footprint: a 9 x 9 grid of its directions
    g = np.linspace(0.0, 1.0, 9)
    rows, sy, cols, sx = np.meshgrid(np.arange(W), g, np.arange(W), g, indexing="ij")
    c = _incidence_cos(basis, W, ps, cols, rows, sx, sy)  # [row][sy][col][sx]
    assert c.min() > 0.1 and c.max() < 0.8  # every primary ray meets the plane, from 37 to 84 degrees
    F = fresnel_cos(c, 1.5)
    Fmin, Fmax = F.min(axis=(1, 3)), F.max(axis=(1, 3))
    Fc = fresnel_cos(_incidence_cos(basis, W, ps, np.arange(W)[None, :], np.arange(W)[:, None], 0.5, 0.5), 1.5)
    L = np.array(SKY)
    tol = (Fmax - Fmin)[:, :, None] * L + L / n + 1e-12
    err = np.abs(img - Fc[:, :, None] * L)
    assert np.all(err <= tol), (err / tol).max()
    assert st["dielectric_reflections"] + st["dielectric_transmissions"] == W * W * n
    assert st["emissive_hits"] == st["dielectric_reflections"] and st["misses"] == st["dielectric_transmissions"]
    assert 0.05 < st["dielectric_reflections"] / (W * W * n) < 0.6
    # flipped: the camera is on the glass side; beyond the critical angle every sample reflects totally
    with flux.Renderer(_fresnel_scene(flux, -1.0, W, ps), flux.JobConfiguration(root, 3, 50), seed=5) as r:
        r.set_math(math_mode(flux, math_name))
        r.enable_stats(True)
        img2 = r.render_frame()
        st2 = r.stats()
    assert np.degrees(np.arccos(c.max())) > np.degrees(np.arcsin(1 / 1.5))
    assert np.all(img2 == L[None, None, :])
    assert st2["dielectric_reflections"] == W * W * n and st2["dielectric_transmissions"] == 0


# ---- 3. the furnace --------------------------------------------------------------------------------------------------

def _cube(c, h, mat):
    from flux_amd.scene import MeshData
    v = np.array([[x, y, z] for x in (-h, h) for y in (-h, h) for z in (-h, h)]) + np.asarray(c)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tris = []
    for a, b, cc, dd in quads:
        tris += [(a, b, cc), (a, cc, dd)]
    tris = np.array(tris, dtype=np.uint32)
    # outward winding: normalize(e1 x e2) points away from the centre
    e1 = v[tris[:, 1]] - v[tris[:, 0]]
    e2 = v[tris[:, 2]] - v[tris[:, 0]]
    ctr = v[tris].mean(axis=1) - np.asarray(c)
    tris[np.einsum("ij,ij->i", np.cross(e1, e2), ctr) < 0] = tris[np.einsum("ij,ij->i", np.cross(e1, e2), ctr) < 0][:, [0, 2, 1]]
    e1 = v[tris[:, 1]] - v[tris[:, 0]]
    e2 = v[tris[:, 2]] - v[tris[:, 0]]
    assert np.all(np.einsum("ij,ij->i", np.cross(e1, e2), ctr) > 0)
    return MeshData(v, tris, mat)


def _furnace(flux, W=48):
    white = flux.EmissiveData((1.0, 1.0, 1.0), 1.0)
    shapes = [flux.SphereData((0.0, 0.0, 0.0), 10.0, white, True),
              flux.SphereData((-1.6, 0.3, 0.0), 1.0, flux.DielectricData(1.5, (1.0, 1.0, 1.0)), False),
              flux.DiskData((0.0, -1.2, 0.5), (0.2, 1.0, -0.1), 1.2, flux.DielectricData(1.5, (1.0, 1.0, 1.0))),
              _cube((1.5, 0.2, 0.3), 0.8, flux.DielectricData(1.33, (1.0, 1.0, 1.0)))]
    return flux.SceneData("furnace", flux.OutputSettings(W, W, 4.0 * 48 / W), (0.0, 0.0, 0.0), shapes,
                          flux.CameraSettings((0.0, 1.0, -6.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)), flux.CameraData(1.0, 100.0, 100.0, 0.0))


@pytest.mark.parametrize("math_name", ["fast", "strict"])
def test_white_furnace(flux, math_name):
    """Every weight is 1 and everything ends on the white environment: a sample is exactly 1, or 0 when the depth limit ends it
    (max_trace_depth 32; STRICT 24, the deepest its per-lane recursion stack holds beside this mesh's BVH stack)."""
    W, root = 48, 8
    n = root * root
    depth = 32 if math_name == "fast" else 24
    img, st, plan = render(flux, _furnace(flux, W), root, math_mode(flux, math_name), depth=depth)
    assert img.max() <= 1.0 + 1e-12
    lit = np.round(img[:, :, 0] * n)
    assert np.all(img[:, :, 0] == img[:, :, 1]) and np.all(img[:, :, 0] == img[:, :, 2])
    assert np.abs(img[:, :, 0] * n - lit).max() < 1e-9
    assert int(lit.sum()) + st["depth_exhausted"] == W * W * n
    assert np.mean(img == 1.0) >= 0.99
    assert st["dielectric_transmissions"] > W * W * n // 20 and st["dielectric_reflections"] > 1000


# ---- 4. the kernels agree ------------------------------------------------------------------------------------------

def _glass_mesh(flux):
    sd = _glass()
    sd.shapes.append(_cube((-2.5, 1.0, 1.5), 0.7, flux.DielectricData(1.45, (0.9, 1.0, 0.8))))
    return sd


@pytest.mark.parametrize("math_name", ["fast", "strict"])
def test_static_refill_split_agree(flux, demo2, switches, math_name):
    sd = _glass()
    m = math_mode(flux, math_name)
    n = 16
    base, sbase, _ = render(flux, sd, n, m, flux.KERNEL_STATIC)
    assert sbase["dielectric_reflections"] > 0 and sbase["dielectric_transmissions"] > 0
    for kernel in (flux.KERNEL_REFILL, flux.KERNEL_SPLIT):
        for cap in (None, "0", "96"):
            switches(FLUX_SPLIT_HITQ_CAP=cap)
            img, st, plan = render(flux, sd, n, m, kernel)
            assert st == sbase, (kernel, cap, st, sbase)
            assert np.abs(img - base).max() <= 1e-12, (kernel, cap)
    switches()
    if math_name == "fast":
        # the launch plan reports what runs: a glass scene keeps the split kernel's ray queue (the LDS of the queue-less plan, which
        # a hit queue would enlarge), where demo2 parks its hits (at 16384 spp: four waves per pixel leave the queue its slots)
        n = 128
        plans = {}
        for name, s in (("glass", sd), ("demo2", small_scene(demo2, 64, 48))):
            for cap in (None, "0"):
                switches(FLUX_SPLIT_HITQ_CAP=cap)
                with flux.Renderer(s, flux.JobConfiguration(n, 5, 50), seed=1) as r:
                    plans[name, cap] = r.launch_plan()
        switches()
        assert plans["glass", None]["kernel"] == flux._lib.PLAN_SPLIT
        assert plans["glass", None] == plans["glass", "0"]
        assert plans["demo2", None]["lds"] > plans["demo2", "0"]["lds"]


@pytest.mark.parametrize("math_name", ["fast", "strict"])
def test_bvh_kernels_agree(flux, math_name):
    sd = _glass_mesh(flux)
    m = math_mode(flux, math_name)
    n = 8
    base, sbase, pbase = render(flux, sd, n, m, traversal=flux._lib.TRAVERSE_BRUTE)
    assert sbase["dielectric_transmissions"] > 0
    plans = set()
    for traversal in (flux._lib.TRAVERSE_BVH, flux._lib.TRAVERSE_BVH_BINARY):
        img, st, plan = render(flux, sd, n, m, traversal=traversal)
        plans.add(plan["kernel"])
        keys = [k for k in st if k not in ("bvh_nodes", "tris_tested")]
        assert {k: st[k] for k in keys} == {k: sbase[k] for k in keys}, traversal
        assert np.abs(img - base).max() <= 1e-12, traversal
    if math_name == "fast":
        assert plans == {flux._lib.PLAN_BVH4, flux._lib.PLAN_BVH_BINARY}


@pytest.mark.parametrize("mesh", [False, True])
def test_fast_against_strict(flux, mesh):
    sd = _glass_mesh(flux) if mesh else _glass()
    a, sa, _ = render(flux, sd, 8, flux.MATH_FAST)
    b, sb, _ = render(flux, sd, 8, flux.MATH_STRICT)
    assert np.abs(a - b).max() < 1e-4
    for k in ("dielectric_reflections", "dielectric_transmissions", "emissive_hits", "misses"):
        assert abs(sa[k] - sb[k]) <= 1e-5 * sa["samples"], k


# ---- 5. shares and loopback ranks ------------------------------------------------------------------------------------

def test_set_shares_row_tiles_and_loopback_ranks(flux):
    sd = _glass((50, 37))
    cfg = flux.JobConfiguration(8, 5, 50)
    with flux.Renderer(sd, cfg, seed=11) as r:
        want = r.render_frame()
        assert np.array_equal(row_tiles(r, 9), want)
        for world in (1, 2, 3):
            assert np.array_equal(set_sharded_frame(flux, r, world).numpy(), want), world
    for G, _, frame in loopback_frames(flux, sd, cfg, 11, (2,), (flux.SHARD_SETS,)):
        assert np.array_equal(frame, want), G


# ---- 6. refractive index 1 -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("math_name", ["fast", "strict"])
def test_index_one_changes_nothing(flux, demo2, math_name):
    """Emitters only (demo2's environment and sphere light): a glass sphere of index 1 and white transmission in front of the light
    passes every ray straight on (F = 0 < u), so the frame is the frame without it."""
    base = small_scene(demo2, 48, 36)
    base.shapes = base.shapes[:2]
    glass = copy.deepcopy(base)
    glass.shapes.append(flux.SphereData((-1.5, 3.0, 0.0), 1.5, flux.DielectricData(1.0, (1.0, 1.0, 1.0)), False))
    m = math_mode(flux, math_name)
    a, sa, _ = render(flux, base, 8, m)
    b, sb, _ = render(flux, glass, 8, m)
    assert sb["dielectric_reflections"] == 0 and sb["dielectric_transmissions"] > 1000
    assert sb["depth_exhausted"] == 0
    assert np.abs(a - b).max() <= 1e-12


# ---- 7. the CLI ----------------------------------------------------------------------------------------------------

def test_cli_writes_the_python_frame(flux, tmp_path):
    flux_bin, _ = host_bins()
    scene = small_yaml(os.path.join(SCENES, "glass.yml"), tmp_path, 64, 48)
    sd = flux.load_scene(scene)
    assert sd.output_settings.image_width == 64 and isinstance(sd.shapes[3].material, flux.DielectricData)
    with flux.Renderer(sd, flux.JobConfiguration(3, 5, 16), seed=5) as r:
        want_img = r.render_frame()
    flux.write_ppm(str(tmp_path / "want.ppm"), want_img)
    got = cli_frame(flux_bin, scene, ["-r", "3", "-d", "5", "-R", "16", "--seed", "5"], tmp_path / "out")
    assert got == open(tmp_path / "want.ppm", "rb").read()
