"""The scenes, jobs and expected launch-plan flags of the split-kernel sweep (tests/test_split_sweep.py on the CPU,
tests/test_gpu_split_sweep.py on the GPU).  Plain functions, as tests/extension_checks.py: no fixtures.

The split kernel (render_body.inc render_split_kernel) is chosen by the launch planner (flux_amd/csrc/launch_plan.cpp) in many
instantiations -- TYP, MAX32, the first plane's axis, hit queue or ray queue, throughput table or multiply loop, the depth cut, the
copy with the dielectric lobe, 1, 2 or 4 waves a pixel -- and the rest of the suite reaches most of them only on demo2 and scenes
made from it by hand.  Here every CLASS of scene is built by a generator of its own, `generator(flux, base, rng, frame, index)`: a
scene is in its class by construction, never by filtering a general stream (the two extension classes too: six scenes of
test_gpu_ext_fuzz.random_ext_scene with a box and a disk needed 30 replaced draws, mostly for frames that see no bounce at all).
All plane and disk normals are unit vectors (FLUX_MATH_FAST is defined for such scenes only), cameras stay inside the environment where there is one, the lens radius is drawn from {0, 0.05, 0.3}.

Scene `index` of a class is draw DRAWS[class][index] of default_rng(BASE[class] + index), 0 unless an earlier draw was not worth
rendering (tests/test_split_sweep.py states the conditions, judges every draw up to the one used by the oracle alone, and caps the
replaced draws at one in four a class).  Its frame is FRAMES[index % 6]; it runs HEADLINE_JOB (root 128, depth 5: four waves a
pixel) and JOBS[index % 6].

expected_flags() restates the planner's rules (plan_hitq, tput_table_bytes, split_typ, split_cut_depth) in Python for K waves a
pixel.  The plan has the last word: every GPU run asserts that launch_plan(flags=True)["flags"] agrees."""
import copy
import functools
import os

import numpy as np

import split_checks as sc
from conftest import SCENES
from split_checks import SLOT, scene_lds

SCENES_PER_CLASS = int(os.environ.get("FLUX_SPLIT_SWEEP_SCENES", "6"))   # a longer sweep: FLUX_SPLIT_SWEEP_SCENES=60
CLASSES = ("typ_axis", "typ_no_axis", "records_17_30", "spheres_33_64", "no_env_shortcut", "beyond_the_guard", "five_exponents",
           "disks_and_boxes", "glass")
ORACLE_CLASSES = CLASSES[:7]          # the other two have shapes and a material the oracle does not know: tests/path_spec.py
BASE = {c: 31000 + 1000 * k for k, c in enumerate(CLASSES)}
# odd widths: map_wave deals an odd set count over the eight XCD slots
FRAMES = ((2, 2), (3, 2), (5, 3), (4, 3), (7, 3), (8, 6))
HEADLINE_JOB = (128, 5)
# (sample root, depth limit): K = 1 with 64 full batches; 4225 spp, a last batch of one sample (4 bits x 8 = 32: the hit queue, no
# table); K = 2, bounce lists of one entry; 16129 spp, K = 2, slices that are no multiple of 64; no hit can be parked; a deep job
JOBS = ((64, 3), (65, 8), (91, 2), (127, 5), (128, 1), (128, 8))
# which draw of its stream a scene is (default 0): the draws before it fail a condition of tests/test_split_sweep.py, which says which
DRAWS = {"typ_no_axis": {1: 1}, "spheres_33_64": {4: 1}, "beyond_the_guard": {1: 1}, "disks_and_boxes": {0: 1}, "glass": {0: 1}}

EXPONENTS = (0.0, 1.0, 2.5, 10.0, 100.0, 1e4)
FIVE_EXPONENTS = (0.0, 1.0, 10.0, 100.0, 1e4)   # more than kGlossExpSlots = 4
AXES = ((1.0, 0.0, 0.0), (-1.0, -0.0, 0.0), (-0.0, 1.0, 0.0), (0.0, -1.0, -0.0), (0.0, -0.0, 1.0), (-0.0, 0.0, -1.0))


def jobs_of(index):
    return (HEADLINE_JOB, JOBS[index % len(JOBS)])


def waves_per_pixel(root):
    """launch_plan.cpp waves_per_pixel: 4096 samples a wave at least, four waves at most"""
    n = root * root
    return 4 if n >= 16384 else 2 if n >= 8192 else 1


# ---- the generators -----------------------------------------------------------------------------------------------------------

def _f3(v):
    return tuple(float(x) for x in v)


def _unit(v):
    """v normalised so that |n.n - 1| <= 4 eps, the library's rule for a unit normal"""
    v = np.asarray(v, dtype=np.float64)
    v = v / np.linalg.norm(v)
    v = v / np.linalg.norm(v)
    assert abs(float(np.dot(v, v)) - 1.0) <= 4.0 * 2.220446049250313e-16
    return _f3(v)


def _color(rng, lo=0.0):
    return _f3(rng.uniform(lo, 1.0, 3))


def _material(flux, rng, exponents, emissive=0.12):
    """Matte, Reflective and Glossy mostly, an emitter now and then: bounces for the queue to park"""
    u = rng.uniform()
    if u < emissive:
        return flux.EmissiveData(_color(rng), float(rng.uniform(0.5, 4.0)))
    if u < 0.5:
        return flux.MatteData(_color(rng, 0.2), _color(rng), float(rng.uniform(0.3, 1.0)))
    if u < 0.7 or not exponents:
        return flux.ReflectiveData(float(rng.uniform(0.3, 1.0)), _color(rng, 0.2))
    return flux.GlossyReflectiveData(float(rng.uniform(0.3, 1.0)), _color(rng, 0.2), float(rng.choice(exponents)))


def _palette(rng):
    """at most 3 distinct glossy exponents a scene"""
    return tuple(float(x) for x in rng.choice(EXPONENTS, size=int(rng.integers(1, 4)), replace=False))


def _camera(sd, rng, frame, up_side=None, look_at=(0.0, 0.0, 0.0), distance=(8.0, 13.0)):
    """The eye 8 to 13 from the origin -- inside every environment sphere drawn here (radius 20 at least) --, on the side `up_side`
    points to where that is given (a floor's normal) and 3 to 30 degrees above that floor, so that most frames see the horizon;
    looking at `look_at`; about 35 degrees across the longer side of the frame."""
    W, H = frame
    sd.output_settings.image_width, sd.output_settings.image_height = W, H
    sd.output_settings.pixel_size = float(rng.uniform(260.0, 380.0)) / max(W, H)
    d = rng.normal(size=3)
    d = d / np.linalg.norm(d)
    if up_side is not None:
        n = np.asarray(up_side, dtype=np.float64)
        flat = d - float(np.dot(d, n)) * n
        d = flat / np.linalg.norm(flat) + float(rng.uniform(0.05, 0.6)) * n
        d = d / np.linalg.norm(d)
    eye = d * float(rng.uniform(*distance))
    sd.camera_settings.eye = _f3(eye)
    sd.camera_settings.look_at = _f3(look_at)
    view = np.asarray(look_at) - eye
    view = view / np.linalg.norm(view)
    sd.camera_settings.up = (0.0, 1.0, 0.0) if abs(view[1]) < 0.9 else (1.0, 0.0, 0.0)
    sd.camera_data.lens_radius = float(rng.choice([0.0, 0.05, 0.3]))
    sd.camera_data.focal_distance = float(rng.uniform(6.0, 12.0))
    sd.camera_data.zoom_factor = 1.0
    sd.background = (0.0, 0.0, 0.0)


def _environment(flux, rng):
    return flux.SphereData((0.0, 0.0, 0.0), float(rng.uniform(20.0, 200.0)), flux.EmissiveData(_color(rng, 0.3), 1.0), True)


def _spheres(flux, rng, count, exponents, reach=5.0, radii=(0.3, 2.0), materials=None, lamp=False):
    """`lamp`: the first one is a small light where the camera looks (a job of depth limit 1 sees nothing but emitters)"""
    out = []
    for k in range(count):
        m = materials[k] if materials is not None and k < len(materials) else _material(flux, rng, exponents)
        out.append(flux.SphereData(_f3(rng.uniform(-reach, reach, 3)), float(rng.uniform(*radii)), m, False))
    if lamp and materials is None:
        out[0] = flux.SphereData(_f3(rng.uniform(-0.5, 0.5, 3)), float(rng.uniform(0.4, 0.9)),
                                 flux.EmissiveData(_color(rng, 0.3), float(rng.uniform(1.0, 4.0))), False)
    return out


def _floor(flux, rng, normal):
    """a Matte plane 1 to 2.5 below the origin along its normal"""
    n = np.asarray(normal, dtype=np.float64)
    return flux.PlaneData(_f3(-n * float(rng.uniform(1.0, 2.5)) + 0.0), _f3(normal),
                          flux.MatteData(_color(rng, 0.3), _color(rng), float(rng.uniform(0.5, 1.0))))


def _tilted_planes(flux, rng, count, exponents, eye):
    """unit planes on no axis, 3 to 6 from the origin, facing it and the eye"""
    out = []
    for _ in range(count):
        n = np.asarray(_unit(rng.normal(size=3)))
        if float(np.dot(n, eye)) < 0.0:
            n = -n
        out.append(flux.PlaneData(_f3(-n * float(rng.uniform(3.0, 6.0))), _f3(n), _material(flux, rng, exponents, emissive=0.0)))
    return out


def _analytic(flux, base, rng, frame, index, n_spheres, first_plane, more_planes, exponents=None, materials=None, reach=5.0,
              radii=(0.3, 2.0), environment=True, lamp=True):
    """An environment, `n_spheres` ordinary spheres, then the planes: `first_plane` is "axis" (AXES[index % 6]), "tilted" or None."""
    sd = copy.deepcopy(base)
    exponents = _palette(rng) if exponents is None else exponents
    shapes = [_environment(flux, rng)] if environment else []
    shapes += _spheres(flux, rng, n_spheres, exponents, reach, radii, materials, lamp=lamp)
    floor_normal = None
    if first_plane == "axis":
        floor_normal = AXES[index % 6]
        shapes.append(_floor(flux, rng, floor_normal))
    elif first_plane == "tilted":
        floor_normal = _unit(rng.normal(size=3))
        shapes.append(_floor(flux, rng, floor_normal))
    _camera(sd, rng, frame, up_side=floor_normal)
    shapes += _tilted_planes(flux, rng, more_planes, exponents, np.asarray(sd.camera_settings.eye))
    sd.shapes = shapes
    return sd


def typ_axis(flux, base, rng, frame, index):
    planes = int(rng.integers(0, 3))
    return _analytic(flux, base, rng, frame, index, int(rng.integers(3, 13 - planes)), "axis", planes)


def typ_no_axis(flux, base, rng, frame, index):
    if index % 2 == 0:
        return _analytic(flux, base, rng, frame, index, int(rng.integers(3, 13)), "tilted", int(rng.integers(0, 2)))
    return _analytic(flux, base, rng, frame, index, int(rng.integers(8, 13)), None, 0, reach=1.8, radii=(0.8, 1.6), lamp=False)   # no plane at all: a cluster that fills the view


def records_17_30(flux, base, rng, frame, index):
    records = (17, 30, 19, 24, 22, 27)[index % 6] if index < 6 else int(rng.integers(17, 31))
    planes = int(rng.integers(0, 3))
    return _analytic(flux, base, rng, frame, index, records - 2 - planes, "axis", planes, radii=(0.3, 1.2))


def spheres_33_64(flux, base, rng, frame, index):
    # spheres (the environment among them) and planes: 34, 39 and 45 records leave four waves room for the hit queue (45 with the
    # last two slots of it), 47, 58 and 64 do not
    n_sph, planes = ((33, 1), (39, 0), (44, 1), (47, 0), (56, 2), (64, 0))[index % 6] if index < 6 else (int(rng.integers(33, 65)), int(rng.integers(0, 3)))
    return _analytic(flux, base, rng, frame, index, n_sph - 1, "axis" if planes else None, max(planes - 1, 0), radii=(0.3, 1.0))


def no_env_shortcut(flux, base, rng, frame, index):
    case = index % 3
    if case == 0:   # no inverted sphere, a coloured background: the oracle counts misses
        light = flux.EmissiveData(_color(rng, 0.3), 2.0)
        sd = _analytic(flux, base, rng, frame, index, int(rng.integers(4, 12)), "axis", 0, environment=False, materials=[light])
        sd.background = _f3(rng.uniform(0.1, 1.5, 3))
        return sd
    sd = _analytic(flux, base, rng, frame, index, int(rng.integers(4, 12)), "axis", 0)
    if case == 1:   # two nested inverted spheres, the eye inside both
        sd.shapes.insert(1, flux.SphereData(_f3(rng.uniform(-1, 1, 3)), float(rng.uniform(16.0, 18.0)),
                                            flux.EmissiveData(_color(rng, 0.3), 1.0), True))
    else:           # a Matte inverted sphere around an Emissive ball
        sd.shapes[0].material = flux.MatteData(_color(rng, 0.3), _color(rng), float(rng.uniform(0.5, 1.0)))
        sd.shapes[1].material = flux.EmissiveData(_color(rng, 0.3), 3.0)
        sd.shapes[1].radius = float(rng.uniform(1.5, 2.0))
    return sd


def beyond_the_guard(flux, base, rng, frame, index):
    """One sphere whose centre or radius lies beyond the 1e3 within which the kernel skips a path's own sphere (self_skip)"""
    if index % 2 == 0:   # a ball of radius 1500 as the ground: centre and radius beyond the guard, and in view
        sd = _analytic(flux, base, rng, frame, index, int(rng.integers(3, 12)), None, 0)
        ground = flux.SphereData((0.0, -1502.0, 0.0), 1500.0, flux.MatteData(_color(rng, 0.3), _color(rng), 0.8), False)
        sd.shapes.append(ground)
        eye = np.asarray(sd.camera_settings.eye)
        eye[1] = abs(eye[1]) + 2.0
        sd.camera_settings.eye = _f3(eye)
        return sd
    sd = _analytic(flux, base, rng, frame, index, int(rng.integers(3, 11)), "axis", 0)   # a small one far outside the environment
    sd.shapes.insert(2, flux.SphereData((2000.0, 0.0, 0.0), 1.0, flux.MatteData(_color(rng), _color(rng), 0.8), False))
    return sd


def five_exponents(flux, base, rng, frame, index):
    glossy = [flux.GlossyReflectiveData(float(rng.uniform(0.4, 1.0)), _color(rng, 0.3), e) for e in FIVE_EXPONENTS]
    return _analytic(flux, base, rng, frame, index, int(rng.integers(6, 13)), "axis", int(rng.integers(0, 2)),
                     exponents=FIVE_EXPONENTS, materials=glossy)


def _extension(flux, base, rng, frame, index, glass):
    """Spheres, one or two boxes and one or two disks (unit normals) -- under an Emissive environment sphere and over a floor (even
    indices), or in a Matte inverted box lit by a disk under its ceiling (odd indices: every path goes on until it meets a light or
    the depth limit); `glass`: one or two of the spheres are Dielectric."""
    sd = copy.deepcopy(base)
    exponents = _palette(rng)
    up = (0.0, 1.0, 0.0)
    if index % 2 == 0:
        shapes = [_environment(flux, rng), _floor(flux, rng, up)]
        _camera(sd, rng, frame, up_side=up)
    else:
        half = rng.uniform(9.0, 12.0, 3)
        shapes = [flux.BoxData(_f3(-half), _f3(half), flux.MatteData(_color(rng, 0.3), _color(rng), float(rng.uniform(0.5, 0.9))), True),
                  flux.DiskData((float(rng.uniform(-2, 2)), float(half[1] - 0.5), float(rng.uniform(-2, 2))), (0.0, -1.0, 0.0),
                                float(rng.uniform(3.0, 5.0)), flux.EmissiveData(_color(rng, 0.5), float(rng.uniform(3.0, 6.0))))]
        _camera(sd, rng, frame, up_side=up, distance=(5.0, 7.0))
    spheres = _spheres(flux, rng, int(rng.integers(2, 5)), exponents, reach=3.0, radii=(0.6, 1.8))
    if glass:
        for s in spheres[:int(rng.integers(1, 3))]:
            s.material = flux.DielectricData(float(rng.choice([1.33, 1.5, 2.4, 0.7])), _color(rng, 0.5))
    shapes += spheres
    for _ in range(int(rng.integers(1, 3))):
        c0 = rng.uniform(-4.0, 2.0, 3)
        shapes.append(flux.BoxData(_f3(c0), _f3(c0 + rng.uniform(0.8, 2.5, 3)), _material(flux, rng, exponents, emissive=0.2), False))
    for _ in range(int(rng.integers(1, 3))):
        shapes.append(flux.DiskData(_f3(rng.uniform(-3, 3, 3)), _unit(rng.normal(size=3)), float(rng.uniform(0.8, 2.5)),
                                    _material(flux, rng, exponents, emissive=0.2)))
    sd.shapes = shapes
    return sd


def disks_and_boxes(flux, base, rng, frame, index):
    return _extension(flux, base, rng, frame, index, glass=False)


def glass(flux, base, rng, frame, index):
    return _extension(flux, base, rng, frame, index, glass=True)


GENERATORS = {"typ_axis": typ_axis, "typ_no_axis": typ_no_axis, "records_17_30": records_17_30, "spheres_33_64": spheres_33_64,
              "no_env_shortcut": no_env_shortcut, "beyond_the_guard": beyond_the_guard, "five_exponents": five_exponents,
              "disks_and_boxes": disks_and_boxes, "glass": glass}


@functools.lru_cache(maxsize=None)
def _base():
    import flux_amd as flux
    return flux.load_scene(os.path.join(SCENES, "demo1.yml"))


def draws(cls, index, count):
    """[(scene, seed)] of the first `count` draws of scene `index`'s stream"""
    import flux_amd as flux
    rng = np.random.default_rng(BASE[cls] + index)
    out = []
    for _ in range(count):
        sd = GENERATORS[cls](flux, _base(), rng, FRAMES[index % len(FRAMES)], index)
        out.append((sd, int(rng.integers(1, 1 << 30))))
    return out


@functools.lru_cache(maxsize=None)
def scene(cls, index):
    """(scene, seed) of scene `index` of class `cls`: never written to"""
    return draws(cls, index, DRAWS.get(cls, {}).get(index, 0) + 1)[-1]


# ---- the planner's rules, restated ----------------------------------------------------------------------------------------------

def _records(flux, sd):
    return sum(6 if isinstance(s, flux.BoxData) else 1 for s in sd.shapes)


def plan_hitq(flux, sd, root, depth, env=None):
    """launch_plan.cpp plan_hitq for the job's K waves a pixel: (C, H, bits an entry), C = 0 for the ray queue"""
    env = env or {}
    K = waves_per_pixel(root)
    bits = max(1, (_records(flux, sd) - 1).bit_length())
    if any(isinstance(s.material, flux.DielectricData) for s in sd.shapes):
        return 0, 0, bits
    granules = 128 * K // (4 * 5)                      # FLUX_WPE_SPLIT = 5 waves a SIMD
    per_wave = max(granules * 1280 - scene_lds(flux, sd) - 96, 0) // K
    cap = (per_wave // SLOT) & ~1
    if "FLUX_SPLIT_HITQ_CAP" in env:
        cap = min(cap, max(0, int(env["FLUX_SPLIT_HITQ_CAP"])) & ~1)
    th = min(64, cap - 64) if cap > 64 + 32 else 32   # FLUX_HITQ_MIN_TAKE = 32
    if "FLUX_SPLIT_HITQ_TAKE_AT" in env:
        th = max(1, min(64, int(env["FLUX_SPLIT_HITQ_TAKE_AT"])))
    if cap >= 64 + th and bits * depth <= 32:
        return cap, th, bits
    return 0, 0, bits


def tput_table_bytes(flux, sd, root, depth, env=None):
    """launch_plan.cpp tput_table_bytes: the bytes of the throughput table a context of the job builds on the host, 0 for none"""
    cap, _, bits = plan_hitq(flux, sd, root, depth, env)
    if root * root < 64 or depth < 2 or cap == 0:
        return 0
    list_bits = bits * (depth - 1)
    size = (2 << list_bits) * 24
    return size if list_bits + 1 <= 24 and size <= (4 << 20) else 0


def _first_plane_axis(flux, sd):
    plane = next((s for s in sd.shapes if isinstance(s, flux.PlaneData)), None)
    if plane is None:
        return 0
    n = [abs(x) for x in plane.normal]
    return {(1.0, 0.0, 0.0): 1, (0.0, 1.0, 0.0): 2, (0.0, 0.0, 1.0): 3}.get(tuple(n), 0)


def split_typ(flux, sd, env=None):
    """launch_plan.cpp split_typ for a scene of unit normals"""
    env = env or {}
    spheres = [s for s in sd.shapes if isinstance(s, flux.SphereData)]
    inverted = [s for s in spheres if s.invert]
    exponents = {s.material.reflect_exponent for s in sd.shapes if isinstance(s.material, flux.GlossyReflectiveData)}
    lobe_table = len(exponents) <= 4 and env.get("FLUX_SAMPLE_TABLES") != "0"
    guard = all(max(abs(x) for x in s.center) < 1e3 and s.radius * s.radius < 1e6 for s in spheres)
    return (len(spheres) <= 32 and guard and len(inverted) == 1 and isinstance(inverted[0].material, flux.EmissiveData) and
            all(isinstance(s, (flux.SphereData, flux.PlaneData)) for s in sd.shapes) and
            not any(isinstance(s.material, flux.DielectricData) for s in sd.shapes) and (not exponents or lobe_table))


def expected_flags(flux, sd, root, depth, env=None):
    """The word launch_plan(flags=True)["flags"] must hold for a FAST split launch of the job, `env` the switches set at context creation"""
    L = flux._lib
    env = env or {}
    cap, _, bits = plan_hitq(flux, sd, root, depth, env)
    table = tput_table_bytes(flux, sd, root, depth, env) > 0    # (every weight drawn here is finite: the table's products are)
    typ = split_typ(flux, sd, env)
    glassy = any(isinstance(s.material, flux.DielectricData) for s in sd.shapes)
    f = (2 if glassy else 1) << L.PLAN_FLAG_COPY_SHIFT
    if typ:
        f |= L.PLAN_FLAG_TYP
        if env.get("FLUX_PLANE_AXIS") != "0":
            f |= _first_plane_axis(flux, sd) << L.PLAN_FLAG_AXIS_SHIFT
    if sum(isinstance(s, flux.SphereData) for s in sd.shapes) <= 32:
        f |= L.PLAN_FLAG_MAX32
    if cap:
        f |= L.PLAN_FLAG_HITQ | bits << L.PLAN_FLAG_HQ_BITS_SHIFT
        if table and env.get("FLUX_THROUGHPUT_TABLE") != "0":
            f |= L.PLAN_FLAG_TPUT_TABLE
    if env.get("FLUX_SPLIT_DEPTH_CUT") != "0" and (cap == 0 or table):
        f |= L.PLAN_FLAG_DEPTH_CUT
    if env.get("FLUX_SPLIT_UNIFORM_A") != "0":
        f |= L.PLAN_FLAG_UNIFORM_A
    return f


def describe(flux, flags):
    L = flux._lib
    names = [n for n, m in (("typ", L.PLAN_FLAG_TYP), ("max32", L.PLAN_FLAG_MAX32), ("hitq", L.PLAN_FLAG_HITQ),
                            ("table", L.PLAN_FLAG_TPUT_TABLE), ("cut", L.PLAN_FLAG_DEPTH_CUT), ("uniform_a", L.PLAN_FLAG_UNIFORM_A)) if flags & m]
    return "|".join(names) + f" axis {(flags & L.PLAN_FLAG_AXIS_MASK) >> L.PLAN_FLAG_AXIS_SHIFT}" \
                             f" bits {(flags & L.PLAN_FLAG_HQ_BITS_MASK) >> L.PLAN_FLAG_HQ_BITS_SHIFT}" \
                             f" copy {(flags & L.PLAN_FLAG_COPY_MASK) >> L.PLAN_FLAG_COPY_SHIFT}"


# ---- the oracle and the path reference, once a (scene, job) -------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def oracle_run(cls, index, draw, root, depth):
    """(frame, statistics, seconds) of the CPU oracle for a draw of an oracle class at the job's full sample count"""
    import time
    import flux_amd as flux
    from oracle import oracle
    sd, seed = draws(cls, index, draw + 1)[-1]
    t0 = time.perf_counter()
    frame, stats = sc.oracle_run(flux, oracle, sd, root, depth, seed)
    return frame, stats, time.perf_counter() - t0


@functools.lru_cache(maxsize=None)
def path_run(cls, index, draw, depth):
    """The 64-spp PathSpec, its frame made, of a draw of an extension class"""
    import path_spec
    sd, seed = draws(cls, index, draw + 1)[-1]
    spec = path_spec.PathSpec(sd, 8, depth, seed)
    spec.frame().setflags(write=False)
    return spec


# ---- is a draw worth rendering?  (tests/test_split_sweep.py asserts this of every scene; a draw that fails is replaced) -------------

def failed_conditions(cls, index, draw):
    """What makes draw `draw` of scene `index` not worth rendering, judged by the oracle alone (tests/path_spec.py at 64 spp for the
    two extension classes) for both of its jobs; [] if nothing does."""
    import flux_amd as flux
    L = flux._lib
    sd, _ = draws(cls, index, draw + 1)[-1]
    failed = []
    for root, depth in jobs_of(index):
        tag = f"root {root} depth {depth}: "
        if cls in ORACLE_CLASSES:
            frame, st, _ = oracle_run(cls, index, draw, root, depth)
        else:
            spec = path_run(cls, index, draw, depth)
            frame, st = spec.frame(), spec.stats
            if not spec.min_margin() > 1e-9:
                failed.append(tag + f"a decision within {spec.min_margin():.1e} of its threshold")
        bounces = st["matte_bounces"] + st["glossy_bounces"] + st["specular_bounces"]
        if bounces < 0.25 * st["samples"]:
            failed.append(tag + f"{bounces} bounces in {st['samples']} samples: nothing for the queue to park")
        if st["emissive_hits"] == 0:
            failed.append(tag + "no path ends on an emitter")
        if expected_flags(flux, sd, root, depth) & L.PLAN_FLAG_DEPTH_CUT and st["depth_exhausted"] == 0:
            failed.append(tag + "the depth cut has no path to end")
        if cls == "no_env_shortcut" and index % 3 == 0 and st["misses"] == 0:
            failed.append(tag + "no miss")
        finite = frame[np.isfinite(frame)]
        if not (finite.size and float(finite.max() - finite.min()) > 0.01):
            failed.append(tag + "a constant frame")
    return failed
