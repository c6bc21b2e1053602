"""Box shapes (extension, include/flux_abi.h FLUX_SHAPE_BOX) on the device, in every render kernel.

The CPU checker is frozen and knows no box, so the evidence is: rays (flux_debug_shade) against tests/box_spec.py, a mirror box
between six emitters (the normals), closed forms, the same scene with its boxes as 12-triangle cubes, and the equivalence of
the kernels, the hit queue, the sharding and the command-line tools on scenes/box_room.yml."""
import copy
import os

import numpy as np
import pytest

import box_spec
from conftest import SCENES, small_scene
from extension_checks import box_as_mesh as _as_mesh, cli_frame, host_bins, loopback_frames, math_mode, node_frame, render, row_tiles, set_sharded_frame, small_yaml
from switches import switches  # noqa: F401 (the fixture)
from test_box_scene import C0, C1, spec_rays

pytestmark = pytest.mark.gpu

T_MIN = box_spec.T_MIN
BG = (0.1, 0.2, 0.3)
EMIT = (0.7, 0.45, 0.25)
POWER = 2.0
BOX_ROOM = os.path.join(SCENES, "box_room.yml")


def _ray_scene(flux, shapes, bg=BG):
    return flux.SceneData("rays", flux.OutputSettings(8, 8, 1.0), bg, shapes, flux.CameraSettings((0, 0, -5), (0, 0, 0), (0, 1, 0)),
                          flux.CameraData(1.0, 100.0, 100.0, 0.0))


def _ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


# ---- rays against the spec ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rays():
    o, d, kinds = spec_rays(np.random.default_rng(7), 100000)
    want = {inv: box_spec.box_hit(C0, C1, o, d, inv) for inv in (False, True)}
    return o, d, kinds, want


@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("math_name", ["fast", "strict"])
def test_random_rays_against_the_spec(flux, rays, math_name, invert):
    o, d, kinds, want = rays
    hw, tw, nw, face, (t0, t1, tmin, tmax) = want[invert]
    sd = _ray_scene(flux, [flux.BoxData(C0, C1, flux.EmissiveData(EMIT, POWER), invert)])
    with flux.Renderer(sd, flux.JobConfiguration(2, 3, 50), seed=2) as r:
        r.set_math(math_mode(flux, math_name))
        rgb, hit, t = r.debug_shade(o, d, 1, 0, 0)
    keep = np.ones(len(o), bool)
    if math_name == "fast":  # decisions at rounding level may fall either way under FAST's reciprocals: excluded, counted
        keep = ~box_spec.rounding_level(t0, t1, tmin, tmax)
        assert (~keep).sum() <= 1e-3 * len(o)
    assert np.all((hit == 0) | (hit == -1))
    assert np.array_equal(hit[keep] == 0, hw[keep])
    h = keep & hw
    assert h.sum() > 40000 and (keep & ~hw).sum() > 20000
    nan_case = kinds == 3
    assert (h & nan_case).sum() > 1000 and (keep & ~hw & nan_case).sum() > 1000
    if math_name == "strict":
        assert np.array_equal(t[h], tw[h])
    else:
        u = _ulps(t[h], tw[h])
        print("FAST t against the spec: max", u.max(), "ulp; excluded", int((~keep).sum()))
        assert u.max() <= 4
    front = np.sum(nw * d, axis=1) < 0.0  # -n.d > 0 (materials.rs:44)
    L = np.array(EMIT) * POWER
    rgb_w = np.tile(np.array(BG), (len(o), 1))
    rgb_w[hw & front] = L
    rgb_w[hw & ~front] = 0.0
    assert np.array_equal(rgb[keep], rgb_w[keep])
    assert (h & front).sum() > 10000 and (h & ~front).sum() > 10000


# ---- normals: a mirror box between six emitters ---------------------------------------------------------------------------

COLOURS = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 1.0, 0.0), (0.0, 1.0, 1.0), (1.0, 0.0, 1.0)]


@pytest.mark.parametrize("math_name", ["fast", "strict"])
def test_mirror_box_between_six_emitters(flux, math_name):
    """A Reflective box (k = 1, white) inside a cube of six emissive planes, one colour per axis direction: a ray that hits the
    box carries the colour of the plane the spec's mirror direction reaches, for every face."""
    R = 20.0
    planes = []
    for k in range(3):
        for s in (-1.0, 1.0):
            p, nrm = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
            p[k], nrm[k] = s * R, -s  # facing inwards: it emits towards the box
            planes.append(flux.PlaneData(tuple(p), tuple(nrm), flux.EmissiveData(COLOURS[len(planes)], 1.0)))
    box = flux.BoxData(C0, C1, flux.ReflectiveData(1.0, (1.0, 1.0, 1.0)))
    sd = _ray_scene(flux, planes + [box], bg=(0.0, 0.0, 0.0))
    rng = np.random.default_rng(5)
    o, d, kinds = spec_rays(rng, 60000)
    sel = (kinds == 0) & np.all(np.abs(o) < 5.0, axis=1) & ~np.all((o >= np.array(C0) - 1e-3) & (o <= np.array(C1) + 1e-3), axis=1)
    o, d = o[sel], d[sel]
    d /= np.linalg.norm(d, axis=1)[:, None]
    hw, tw, nw, face, (t0, t1, tmin, tmax) = box_spec.box_hit(C0, C1, o, d)
    keep = hw & ~box_spec.rounding_level(t0, t1, tmin, tmax)
    assert set(np.unique(face[keep])) == set(range(6)) and keep.sum() > 3000
    q = o + tw[:, None] * d
    ndotwo = -np.sum(nw * d, axis=1)
    w = d + nw * (ndotwo * 2.0)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        tp = np.stack([((s * R) - q[:, k]) / w[:, k] for k in range(3) for s in (-1.0, 1.0)], axis=1)
    tp[~(tp > T_MIN)] = np.inf
    order = np.sort(tp, axis=1)
    keep &= (order[:, 1] - order[:, 0]) > 1e-6 * order[:, 0]  # away from the outer cube's edges
    want = np.array(COLOURS)[np.argmin(tp, axis=1)]
    with flux.Renderer(sd, flux.JobConfiguration(2, 3, 50), seed=2) as r:
        r.set_math(math_mode(flux, math_name))
        rgb, hit, t = r.debug_shade(o, d, 1, 0, 0)
    assert np.all(hit[keep] == 6)
    if math_name == "strict":
        assert np.array_equal(rgb[keep], want[keep])
    else:
        assert np.abs(rgb[keep] - want[keep]).max() <= 1e-12
    assert len(np.unique(np.argmin(tp, axis=1)[keep])) == 6


def _mirror_room_reference(o, d, centres, radius, depth):
    """numpy's path through an inverted mirror box (weights 1) holding emissive spheres: per ray the index of the sphere it ends on
    (-1: lost to the depth limit), the number of wall bounces before it, the face of its FIRST wall bounce, and whether every
    decision on the way was clear of rounding level."""
    n_rays = len(o)
    end = np.full(n_rays, -1)
    bounces = np.zeros(n_rays, int)
    first_face = np.full(n_rays, -1)
    clear = np.ones(n_rays, bool)
    live = np.ones(n_rays, bool)
    o, d = o.copy(), d.copy()
    for _ in range(depth):
        hb, tb, nb, face, (t0, t1, tmin, tmax) = box_spec.box_hit(C0, C1, o, d, True)
        clear &= ~live | (hb & ~box_spec.rounding_level(t0, t1, tmin, tmax))
        ts = np.full((n_rays, len(centres)), np.inf)
        for k, c in enumerate(centres):
            oc = o - c
            b = np.sum(oc * d, axis=1)
            dq = b * b - (np.sum(oc * oc, axis=1) - radius * radius)
            clear &= ~live | (np.abs(dq) > 1e-6)
            e = np.sqrt(np.maximum(dq, 0.0))
            t = np.where(-b - e > T_MIN, -b - e, -b + e)
            ts[:, k] = np.where((dq >= 0.0) & (t > T_MIN), t, np.inf)
        ks = np.argmin(ts, axis=1)
        tsm = ts[np.arange(n_rays), ks]
        clear &= ~live | (np.abs(tsm - tb) > 1e-6)
        on_sphere = live & (tsm < tb)
        end[on_sphere] = ks[on_sphere]
        live &= ~on_sphere
        first_face = np.where(live & (bounces == 0), face, first_face)
        bounces += live
        q = o + tb[:, None] * d
        w = d + nb * (-np.sum(nb * d, axis=1) * 2.0)[:, None]
        o = np.where(live[:, None], q, o)
        d = np.where(live[:, None], w, d)
    return end, bounces, first_face, clear


@pytest.mark.parametrize("math_name", ["fast", "strict"])
def test_inverted_mirror_room_with_six_emitters_inside(flux, math_name):
    """The same from inside: an inverted Reflective box (its normals point inwards) holding six emissive spheres, one colour in front
    of each face.  A ray from inside carries the colour of the sphere its chain of mirror directions -- about the spec's inward
    face normals -- reaches, or nothing when the depth limit comes first; every face is the first bounce of rays that end on a sphere.
    (A mirror direction tells the normal's axis, not its sign: the sign of every face, for both `invert` values and from both
    sides, is what the emissive front / back radiance of test_random_rays_against_the_spec checks.)"""
    c0, c1 = np.array(C0), np.array(C1)
    mid, ext = 0.5 * (c0 + c1), c1 - c0
    radius, depth = 0.22, 4
    centres = []
    for k in range(3):
        for s in (-1.0, 1.0):
            c = mid.copy()
            c[k] += s * (0.5 * ext[k] - 0.36)
            centres.append(c)
    shapes = [flux.SphereData(tuple(c), radius, flux.EmissiveData(COLOURS[i], 1.0), False) for i, c in enumerate(centres)]
    shapes.append(flux.BoxData(C0, C1, flux.ReflectiveData(1.0, (1.0, 1.0, 1.0)), True))
    sd = _ray_scene(flux, shapes, bg=(0.0, 0.0, 0.0))
    rng = np.random.default_rng(9)
    o = c0 + rng.uniform(0.03, 0.97, (30000, 3)) * ext
    o = o[np.all([np.linalg.norm(o - c, axis=1) > radius + 0.02 for c in centres], axis=0)]
    d = rng.normal(size=(len(o), 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    end, bounces, first_face, clear = _mirror_room_reference(o, d, centres, radius, depth)
    want = np.where((end >= 0)[:, None], np.array(COLOURS)[np.maximum(end, 0)], 0.0)
    with flux.Renderer(sd, flux.JobConfiguration(2, depth, 50), seed=2) as r:
        r.set_math(math_mode(flux, math_name))
        rgb, hit, t = r.debug_shade(o, d, 1, 0, 0)
    via_wall = clear & (end >= 0) & (bounces >= 1)
    assert clear.sum() > 0.9 * len(o)
    for face in range(6):
        assert (via_wall & (first_face == face)).sum() >= 200, face
    assert (clear & (end < 0)).sum() > 100 and (via_wall & (bounces >= 2)).sum() > 500
    if math_name == "strict":
        assert np.array_equal(rgb[clear], want[clear])
    else:
        assert np.abs(rgb[clear] - want[clear]).max() <= 1e-12


# ---- closed forms ---------------------------------------------------------------------------------------------------------

def _camera_scene(flux, shapes, W=16, H=12, eye=(0.0, 0.0, -5.0), bg=(0.0, 0.0, 0.0), ps=1.0, vpd=40.0):
    return flux.SceneData("box", flux.OutputSettings(W, H, ps), bg, shapes, flux.CameraSettings(eye, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)),
                          flux.CameraData(1.0, vpd, vpd, 0.0))


@pytest.mark.parametrize("math_name", ["fast", "strict"])
def test_closed_forms(flux, math_name):
    m = math_mode(flux, math_name)
    L = np.array([0.5, 0.25, 0.125])  # exactly representable, below 1: the mean of N equal samples is L exactly
    emis = flux.EmissiveData((0.5, 0.25, 0.125), 1.0)
    room = _camera_scene(flux, [flux.BoxData((-7.0, -6.0, -9.0), (7.0, 6.0, 9.0), emis, True)])
    for n, kernel in ((4, flux.KERNEL_STATIC), (8, flux.KERNEL_REFILL), (16, flux.KERNEL_SPLIT)):
        img, st, _ = render(flux, room, n, m, kernel)
        assert np.array_equal(img, np.broadcast_to(L, img.shape)), (n, kernel)
        assert st["emissive_hits"] == st["samples"] == 16 * 12 * n * n
        dark = copy.deepcopy(room)
        dark.shapes[0].invert = False  # seen from inside, an outward emitter is black
        img, st, _ = render(flux, dark, n, m, kernel)
        assert np.all(img == 0.0) and st["emissive_hits"] == st["samples"]
    # a silhouette: the box's front face z = -1 (the back face projects inside it), the pinhole at z = -5 on the axis
    W, H, ps, vpd = 16, 12, 1.0, 40.0
    c0, c1 = (-0.83, -0.41, -1.0), (0.57, 0.66, 1.0)
    sd = _camera_scene(flux, [flux.BoxData(c0, c1, emis)], W, H, ps=ps, vpd=vpd)
    img, _, _ = render(flux, sd, 16, m, flux.KERNEL_SPLIT)
    # pixel (row, col): u in ps (col - W/2 + [0, 1]), v in ps ((H - row) - H/2 + [0, 1]); direction (-u, v, vpd): x = -u 4 / vpd, y = v 4 / vpd
    sc = 4.0 / vpd
    x_hi = -ps * (np.arange(W) - W / 2) * sc
    x_lo = -ps * (np.arange(W) - W / 2 + 1) * sc
    y_lo = ps * ((H - np.arange(H)) - H / 2) * sc
    y_hi = ps * ((H - np.arange(H)) - H / 2 + 1) * sc
    in_x, out_x = (x_lo > c0[0]) & (x_hi < c1[0]), (x_hi < c0[0]) | (x_lo > c1[0])
    in_y, out_y = (y_lo > c0[1]) & (y_hi < c1[1]), (y_hi < c0[1]) | (y_lo > c1[1])
    inside = in_y[:, None] & in_x[None, :]
    outside = out_y[:, None] | out_x[None, :]
    assert inside.sum() >= 100 and outside.sum() >= 24  # two whole columns lie right of the face
    assert np.array_equal(img[inside], np.broadcast_to(L, img[inside].shape)) and np.all(img[outside] == 0.0)


@pytest.mark.parametrize("math_name", ["fast", "strict"])
def test_white_furnace(flux, math_name):
    """An inverted emissive room holding a mirror box (k = 1) and a glass box (transmit colour 1): every sample carries L or is lost
    to the depth limit, so the frame's deficit is the statistics' depth_exhausted count."""
    L, n, W, H = 0.5, 16, 16, 12
    shapes = [flux.BoxData((-6.0, -5.0, -8.0), (6.0, 5.0, 8.0), flux.EmissiveData((L, L, L), 1.0), True),
              flux.BoxData((-2.4, -1.3, -0.7), (-0.4, 0.9, 1.1), flux.ReflectiveData(1.0, (1.0, 1.0, 1.0))),
              flux.BoxData((0.3, -1.1, -0.5), (2.2, 1.2, 1.3), flux.DielectricData(1.5, (1.0, 1.0, 1.0)))]
    sd = _camera_scene(flux, shapes, W, H, vpd=25.0)
    img, st, _ = render(flux, sd, n, math_mode(flux, math_name), depth=6)
    assert np.all(img[:, :, 0] == img[:, :, 1]) and np.all(img[:, :, 0] == img[:, :, 2])
    lost = np.rint((1.0 - img[:, :, 0] / L) * n * n)
    assert np.abs((1.0 - img[:, :, 0] / L) * n * n - lost).max() < 1e-9  # every sample is L or 0
    assert int(lost.sum()) == st["depth_exhausted"] and st["misses"] == 0
    assert st["emissive_hits"] + st["depth_exhausted"] == st["samples"] == W * H * n * n
    assert st["specular_bounces"] > 1000 and st["dielectric_transmissions"] > 1000 and st["dielectric_reflections"] > 10


# ---- box against 12-triangle cube -----------------------------------------------------------------------------------------

QUEUE_BYTES = 9 * 64 * 8 + 2 * 64 * 4  # a wave's ray queue (flux_plan.h kQueueBytesPerWave)
HITQ_SLOT_BYTES = 7 * 8 + 3 * 4        # a hit queue slot (kHitQBytesPerSlot)
ROOM_RECORDS = 20 * 96 + 32            # box_room in LDS: 1 sphere + 1 disk + 3 x 6 faces, and the one scan sphere


def _box_room(flux, w=16, h=12):
    return small_scene(flux.load_scene(BOX_ROOM), w, h)


def _glass_room(flux, w=16, h=12):
    sd = _box_room(flux, w, h)
    sd.shapes[3].material = flux.DielectricData(1.5, (0.9, 1.0, 0.95))
    # lifted off the floor: as meshes, the block's bottom and the floor under it would be coplanar triangles whose distances differ by ulps
    sd.shapes[3].corner0 = (1.5, 0.01, 0.0)
    return sd


def _meshed(flux, sd):
    s = copy.deepcopy(sd)
    s.shapes = [_as_mesh(flux, x) if isinstance(x, flux.BoxData) else x for x in s.shapes]
    return s


@pytest.mark.parametrize("math_name", ["fast", "strict"])
def test_box_against_twelve_triangle_cubes(flux, math_name):
    m = math_mode(flux, math_name)
    sd = _glass_room(flux)
    a, sa, pa = render(flux, sd, 16, m)
    b, sb, pb = render(flux, _meshed(flux, sd), 16, m)
    if math_name == "fast":
        assert pa["kernel"] == flux._lib.PLAN_SPLIT and pb["kernel"] == flux._lib.PLAN_BVH4
    diff = np.abs(a - b).max()
    rel = {k: abs(sa[k] - sb[k]) / max(sa[k], 1) for k in sa if k not in ("bvh_nodes", "tris_tested")}
    print("box against cubes:", math_name, "max |difference|", diff, "statistics", rel)
    assert sa["samples"] == sb["samples"]
    assert diff <= 1e-4
    assert all(v <= 1e-4 for v in rel.values()), rel


# ---- kernels, hit queue, sharding, tools ----------------------------------------------------------------------------------

@pytest.mark.parametrize("scene", ["box_room", "glass"])
def test_kernels_agree(flux, scene):
    sd = _box_room(flux) if scene == "box_room" else _glass_room(flux)
    frames = {}
    for kernel in (flux.KERNEL_STATIC, flux.KERNEL_REFILL, flux.KERNEL_SPLIT):
        frames[kernel] = render(flux, sd, 16, flux.MATH_FAST, kernel)
    assert frames[flux.KERNEL_SPLIT][2]["kernel"] == flux._lib.PLAN_SPLIT and frames[flux.KERNEL_REFILL][2]["kernel"] == flux._lib.PLAN_REFILL
    a, sa, _ = frames[flux.KERNEL_STATIC]
    for kernel in (flux.KERNEL_REFILL, flux.KERNEL_SPLIT):
        b, sb, _ = frames[kernel]
        assert sa == sb, (kernel, sa, sb)
        assert np.abs(a - b).max() <= 1e-12, kernel
    s, ss, _ = render(flux, sd, 16, flux.MATH_STRICT)
    assert np.abs(a - s).max() <= 1e-4
    assert ss["samples"] == sa["samples"]


@pytest.mark.parametrize("scene", ["box_room", "glass"])
def test_hit_queue_on_and_off(flux, switches, scene):
    """sample_root 128 on 8 x 6: four waves a pixel, the split kernel with its hit queue (box_room; a scene with glass keeps the ray
    queue either way) against FLUX_SPLIT_HITQ_CAP=0."""
    sd = _box_room(flux, 8, 6) if scene == "box_room" else _glass_room(flux, 8, 6)
    a, sa, pa = render(flux, sd, 128, flux.MATH_FAST)
    switches(FLUX_SPLIT_HITQ_CAP=0)
    b, sb, pb = render(flux, sd, 128, flux.MATH_FAST)
    switches()
    assert pa["kernel"] == pb["kernel"] == flux._lib.PLAN_SPLIT
    assert sa == sb and np.abs(a - b).max() <= 1e-12
    # that the queue was on in the first run shows in the plan's LDS: 4 waves x C slots of 68 B against 4 ray queues of 5 120 B,
    # each beside the records (20 x 96 B and one 32-B scan sphere)
    with flux.Renderer(sd, flux.JobConfiguration(128, 5, 50), seed=1) as r:
        on = r.launch_plan()
        switches(FLUX_SPLIT_HITQ_CAP=0)
        off = r.launch_plan()
        switches()
    assert on["waves_per_pixel"] == off["waves_per_pixel"] == 4 and off["lds"] == 4 * QUEUE_BYTES + ROOM_RECORDS
    if scene == "box_room":
        slots, rest = divmod(on["lds"] - ROOM_RECORDS, 4 * HITQ_SLOT_BYTES)
        assert rest == 0 and slots >= 96 and slots % 2 == 0 and on["lds"] != off["lds"], (on, off)
    else:
        assert on == off  # a scene with glass keeps the ray queue


@pytest.mark.parametrize("scene", ["box_room", "glass"])
def test_set_shares_row_tiles_and_loopback_ranks(flux, scene):
    sd = _box_room(flux, 16, 11) if scene == "box_room" else _glass_room(flux, 16, 11)
    cfg = flux.JobConfiguration(8, 5, 50)
    with flux.Renderer(sd, cfg, seed=11) as r:
        want = r.render_frame()
        assert np.array_equal(row_tiles(r, 4), want)  # row tiles of 4, 4 and 3 rows
        for world in (1, 2, 3):
            assert np.array_equal(set_sharded_frame(flux, r, world).numpy(), want), world
    for G, mode, frame in loopback_frames(flux, sd, cfg, 11, (2, 3), (flux.SHARD_SETS, flux.SHARD_ROWS)):
        assert np.array_equal(frame, want), (G, mode)


@pytest.mark.parametrize("scene_name", ["box_room", "glass"])
def test_cli_and_node_write_the_python_frame(flux, tmp_path, scene_name):
    flux_bin, node_bin = host_bins()
    edits = []
    if scene_name == "glass":  # the polished block as glass, lifted off the floor as in _glass_room
        text = open(BOX_ROOM).read()
        glossy = text[text.index("# A polished block"):text.index("  - Sphere:")]
        glass = glossy[:glossy.index("        GlossyReflective:")] + \
            "        Dielectric:\n          refraction_index: 1.5\n          transmit_color: [0.9, 1.0, 0.95]\n"
        edits = [(glossy, glass), ("corner0: [1.5, 0.0, 0.0]", "corner0: [1.5, 0.01, 0.0]")]
    scene = small_yaml(BOX_ROOM, tmp_path, 16, 12, edits)
    sd = flux.load_scene(scene)
    assert sd.output_settings.image_width == 16 and isinstance(sd.shapes[0], flux.BoxData)
    assert isinstance(sd.shapes[3].material, flux.DielectricData) == (scene_name == "glass")
    with flux.Renderer(sd, flux.JobConfiguration(3, 5, 16), seed=5) as r:
        want_img = r.render_frame()
    flux.write_ppm(str(tmp_path / "want.ppm"), want_img)
    want = open(tmp_path / "want.ppm", "rb").read()
    common = ["-r", "3", "-d", "5", "-R", "16", "--seed", "5"]
    assert cli_frame(flux_bin, scene, common, tmp_path / "direct") == want
    assert node_frame(flux_bin, node_bin, scene, common, tmp_path / "remote", tmp_path) == want


# ---- ties -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("math_name", ["fast", "strict"])
def test_ties_go_to_the_lower_yaml_index(flux, math_name):
    m = math_mode(flux, math_name)
    emis = flux.EmissiveData(EMIT, POWER)
    matte = flux.MatteData((0.5, 0.5, 0.5), (0, 0, 0), 1.0)
    cfg = flux.JobConfiguration(2, 3, 50)
    rng = np.random.default_rng(11)
    # rays straight down onto the top face y = 0.5 of the box, which a plane shares: (0.5 - oy) * (1 / -1) and (0.5 - oy) / -1 are the same bits
    o = np.column_stack([rng.uniform(-0.9, 0.9, 2000), rng.uniform(1.0, 3.0, 2000), rng.uniform(-0.9, 0.9, 2000)])
    d = np.tile([0.0, -1.0, 0.0], (2000, 1))
    box, plane = flux.BoxData((-1.0, -0.5, -1.0), (1.0, 0.5, 1.0), emis), flux.PlaneData((0.3, 0.5, -0.2), (0.0, 1.0, 0.0), matte)
    for shapes in ([box, plane], [plane, box]):
        with flux.Renderer(_ray_scene(flux, shapes), cfg) as r:
            r.set_math(m)
            _, hit, t = r.debug_shade(o, d, 1, 0, 0)
        assert np.all(hit == 0) and np.array_equal(t, o[:, 1] - 0.5)
    # two boxes sharing the face x = 0: a ray inside the first, travelling +x, finds its exit and the second's entry at the same t
    a = flux.BoxData((-1.0, -1.0, -1.0), (0.0, 1.0, 1.0), matte)
    b = flux.BoxData((0.0, -1.0, -1.0), (1.0, 1.0, 1.0), emis)
    o2 = np.column_stack([rng.uniform(-0.9, -0.1, 2000), rng.uniform(-0.9, 0.9, 2000), rng.uniform(-0.9, 0.9, 2000)])
    d2 = np.tile([1.0, 0.0, 0.0], (2000, 1))
    for shapes, first in (([a, b], 0), ([b, a], 0)):
        with flux.Renderer(_ray_scene(flux, shapes), cfg) as r:
            r.set_math(m)
            _, hit, t = r.debug_shade(o2, d2, 1, 0, 0)
        assert np.all(hit == first) and np.array_equal(t, -o2[:, 0])


# ---- launch plans and scenes the box must not touch -----------------------------------------------------------------------

def test_launch_plans(flux, demo2):
    sd = flux.load_scene(BOX_ROOM)
    with flux.Renderer(sd, flux.JobConfiguration(16, 5, 50), seed=1) as r:
        plan = r.launch_plan()
        # 256 spp: one wave a pixel, whose share of the LDS holds no hit queue beside the records: the ray queue.
        # (Which instantiation -- never TYP for a scene with boxes -- is not in this report: tests/box_host_selftest.cpp pins it.)
        assert plan["kernel"] == flux._lib.PLAN_SPLIT and plan["waves_per_pixel"] == 1 and plan["block"] == 64
        assert plan["lds"] == QUEUE_BYTES + ROOM_RECORDS
    with flux.Renderer(small_scene(sd, 8, 6), flux.JobConfiguration(128, 5, 50), seed=1) as r:
        plan = r.launch_plan()  # 16384 spp: four waves a pixel, with the hit queue
        slots, rest = divmod(plan["lds"] - ROOM_RECORDS, 4 * HITQ_SLOT_BYTES)
        assert plan["kernel"] == flux._lib.PLAN_SPLIT and plan["waves_per_pixel"] == 4 and rest == 0 and slots >= 96
    # demo2's plans are what they were: 13 records and 12 scan spheres beside one ray queue at 256 spp; at 16384 spp the hit queue of
    # 110 slots a wave (flux_plan.h: 25 granules of 1 280 B a block, less the records and 96 B, over four waves)
    with flux.Renderer(demo2, flux.JobConfiguration(16, 5, 50), seed=1) as r:
        plan = r.launch_plan()
        assert (plan["kernel"], plan["block"], plan["waves_per_pixel"], plan["lds"]) == (flux._lib.PLAN_SPLIT, 64, 1, QUEUE_BYTES + 13 * 96 + 12 * 32)
    with flux.Renderer(small_scene(demo2, 8, 6), flux.JobConfiguration(128, 5, 50), seed=1) as r:
        plan = r.launch_plan()
        assert (plan["kernel"], plan["block"], plan["waves_per_pixel"], plan["lds"]) == \
            (flux._lib.PLAN_SPLIT, 256, 4, 4 * 110 * HITQ_SLOT_BYTES + 13 * 96 + 12 * 32)
    with flux.Renderer(_meshed(flux, _box_room(flux)), flux.JobConfiguration(16, 5, 50), seed=1) as r:
        assert r.launch_plan()["kernel"] == flux._lib.PLAN_BVH4
    # 200 boxes = 1 200 hit records overflow the split kernel's 16 KiB of LDS: the refill kernel, and the rays still match the spec
    rng = np.random.default_rng(3)
    lo = rng.uniform(-3.0, 2.0, (200, 3))
    ext = rng.uniform(0.2, 1.0, (200, 3))
    many = _ray_scene(flux, [flux.BoxData(tuple(lo[k]), tuple(lo[k] + ext[k]), flux.EmissiveData(EMIT, POWER)) for k in range(200)])
    o = rng.uniform(-6.0, 6.0, (4000, 3))
    d = rng.uniform(-3.0, 3.0, (4000, 3)) - o  # aimed into the cloud of boxes
    best_t = np.full(4000, np.inf)
    best = np.full(4000, -1)
    for k in range(200):
        h, t, _, _, _ = box_spec.box_hit(lo[k], lo[k] + ext[k], o, d)
        take = h & (t < best_t)
        best_t = np.where(take, t, best_t)
        best = np.where(take, k, best)
    assert (best >= 0).sum() > 1000
    with flux.Renderer(many, flux.JobConfiguration(16, 3, 50), seed=1) as r:
        assert r.launch_plan()["kernel"] == flux._lib.PLAN_REFILL
        r.set_math(flux.MATH_STRICT)
        _, hit, t = r.debug_shade(o, d, 1, 0, 0)
        assert np.array_equal(hit, best) and np.array_equal(t[best >= 0], best_t[best >= 0])
        # FAST (hit records up to index 1 199): the same winners wherever the two nearest candidates are not within rounding of
        # each other, t within 4 ulp
        r.set_math(flux.MATH_FAST)
        _, hit, t = r.debug_shade(o, d, 1, 0, 0)
    keep = np.ones(4000, bool)
    second = np.full(4000, np.inf)
    for k in range(200):
        h, tk, _, _, (t0, t1, tmin, tmax) = box_spec.box_hit(lo[k], lo[k] + ext[k], o, d)
        keep &= ~box_spec.rounding_level(t0, t1, tmin, tmax)
        second = np.where(h & (k != best), np.minimum(second, tk), second)
    keep &= ~(np.abs(second - best_t) <= 1e-9 * best_t)
    assert (~keep).sum() <= 40, (~keep).sum()  # 200 boxes' worth of the single box's 1e-3 cap would be 800 of 4 000; a hundredth is ample
    assert np.array_equal(hit[keep], best[keep])
    hk = keep & (best >= 0)
    assert _ulps(t[hk], best_t[hk]).max() <= 4


@pytest.mark.parametrize("math_name", ["fast", "strict"])
def test_out_of_reach_box_changes_nothing(flux, demo2, math_name):
    """demo2 plus a box outside its environment sphere (radius 100), listed second so that every later YAML index moves by one."""
    base = small_scene(demo2, 16, 12)
    far = copy.deepcopy(base)
    far.shapes.insert(1, flux.BoxData((150.0, 150.0, 150.0), (160.0, 170.0, 180.0), flux.EmissiveData((1.0, 0.0, 0.0), 50.0)))
    m = math_mode(flux, math_name)
    for n, kernel in ((4, flux.KERNEL_STATIC), (8, flux.KERNEL_REFILL), (16, flux.KERNEL_SPLIT)):
        a, sa, pa = render(flux, base, n, m, kernel)
        b, sb, pb = render(flux, far, n, m, kernel)
        assert sa == sb and pa["kernel"] == pb["kernel"], (n, kernel)
        print("out of reach:", math_name, n, kernel, "max |difference|", np.abs(a - b).max())
        if math_name == "strict":
            assert np.array_equal(a, b), (n, kernel)
        else:
            assert np.abs(a - b).max() <= 1e-12, (n, kernel)
