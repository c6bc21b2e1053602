"""Differential fuzzing of the extensions: random scenes of spheres, planes, disks, boxes and triangle soups under the five
materials (Dielectric included), rendered by every kernel in both arithmetics and held against tests/path_spec.py, the full-path
reference that tests/test_path_spec.py pins against the CPU restatement before it judges a kernel.  As in tests/test_gpu_fuzz.py
the path statistics must be equal -- all ten -- and nothing is excluded: test_path_spec.py shows that in every scene drawn here no
decision of the reference lies within 1e-9 of its threshold, so a differing count is a decision the kernel took otherwise.

Every fourth scene keeps the generator's non-unit plane and disk normals and must be routed to the STRICT arithmetic; the others
have them normalised after the draw, so the random stream is the same either way."""
import copy
import functools
import os

import numpy as np
import pytest

import aov_spec
import path_spec
import switches
from conftest import SCENES
from split_checks import REC, SLOT, SPH   # a hit record, a hit queue slot, a scan sphere (bytes in LDS)

pytestmark = pytest.mark.gpu

TOL, TOL_TIGHT = 1e-4, 1e-9   # the north-star tolerance; tests/test_gpu_parity.py
REFRACTION_INDICES = [1.0, 1.33, 1.5, 2.4, 0.7]
EXPONENTS = [0.0, 1.0, 10.0, 100.0, 1e4]
CASES = 4                      # scenes a chunk
CHUNKS = int(os.environ.get("FLUX_EXT_FUZZ_CHUNKS", "12"))           # a longer soak: FLUX_EXT_FUZZ_CHUNKS=200
MESH_CHUNKS = int(os.environ.get("FLUX_EXT_FUZZ_MESH_CHUNKS", "4"))
# A chunk's random stream is default_rng(SEED_BASE[mesh] + chunk).  tests/test_path_spec.py demands that no scene of the default
# chunks takes a decision within 1e-9 of its threshold; a chunk that drew one gets another base here (RESEEDED[(mesh, chunk)]).
SEED_BASE = {False: 7000, True: 9000}
RESEEDED = {}


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return tuple(float(x) for x in v / np.linalg.norm(v))


def random_ext_scene(flux, base, rng, unit_normals, frame=None):
    """`unit_normals` normalises the plane and disk normals AFTER the scene is drawn (as tests/test_gpu_fuzz.py random_scene does);
    `frame` = (W, H) overrides the drawn frame size, the stream unchanged."""
    sd = copy.deepcopy(base)
    W, H = int(rng.integers(8, 13)), int(rng.integers(6, 10))
    if frame is not None:
        W, H = frame
    sd.output_settings.image_width, sd.output_settings.image_height = W, H
    sd.output_settings.pixel_size = float(rng.uniform(15.0, 45.0))
    sd.background = tuple(float(x) for x in rng.uniform(0.0, 1.5, 3)) if rng.uniform() < 0.5 else (0.0, 0.0, 0.0)
    eye = rng.uniform(-6, 6, 3)
    eye[1] = abs(eye[1]) + 0.5
    sd.camera_settings.eye = tuple(float(x) for x in eye)
    sd.camera_settings.look_at = tuple(float(x) for x in rng.uniform(-1, 1, 3))
    sd.camera_settings.up = (0.0, 1.0, 0.0) if rng.uniform() < 0.7 else tuple(float(x) for x in rng.normal(size=3))
    sd.camera_data.lens_radius = float(rng.choice([0.0, 0.0, 0.05, 0.3]))
    sd.camera_data.focal_distance = float(rng.uniform(3.0, 12.0))
    sd.camera_data.zoom_factor = float(rng.uniform(0.5, 2.0))

    def color(lo=0.0):
        return tuple(float(x) for x in rng.uniform(lo, 1.0, 3))

    glassy = bool(rng.uniform() < 0.5)   # the other scenes have no glass: the hit queue's (a scene with glass keeps the ray queue)

    def material():
        k = int(rng.integers(0, 6 if glassy else 4))
        if k == 0:
            return flux.MatteData(color(), color(), float(rng.uniform(0.1, 1.0)))
        if k == 1:
            return flux.EmissiveData(color(), float(rng.uniform(0.0, 4.0)))
        if k == 2:
            return flux.ReflectiveData(float(rng.uniform(0.1, 1.0)), color())
        if k == 3:
            return flux.GlossyReflectiveData(float(rng.uniform(0.1, 1.0)), color(), float(rng.choice(EXPONENTS)))
        return flux.DielectricData(float(rng.choice(REFRACTION_INDICES)), color(0.5))   # two draws in six: glass paths are long

    def point(lim):
        return tuple(float(x) for x in rng.uniform(-lim, lim, 3))

    def normal():
        return tuple(float(x) for x in rng.normal(size=3) * rng.choice([0.3, 1.0, 2.5]))  # never normalised by the library

    shapes = []
    room = rng.uniform()
    if room < 0.35:
        shapes.append(flux.SphereData((0.0, 0.0, 0.0), float(rng.uniform(20, 200)), flux.EmissiveData(color(), 1.0), True))
    elif room < 0.7:
        half = rng.uniform(8.0, 30.0, 3)
        shapes.append(flux.BoxData(tuple(float(-x) for x in half), tuple(float(x) for x in half),
                                   flux.EmissiveData(color(), 1.0) if rng.uniform() < 0.7 else material(), True))
    for _ in range(int(rng.integers(2, 14))):
        kind = rng.uniform()
        if kind < 0.35:
            r = float(rng.choice([rng.uniform(0.05, 0.3), rng.uniform(0.3, 2.0), rng.uniform(2.0, 8.0)]))
            shapes.append(flux.SphereData(point(5), r, material(), bool(rng.uniform() < 0.15)))
        elif kind < 0.5:
            shapes.append(flux.PlaneData(point(3), normal(), material()))
        elif kind < 0.75:
            r = float(rng.choice([0.0, rng.uniform(0.3, 3.0), rng.uniform(0.3, 3.0), rng.uniform(3.0, 30.0)]))
            shapes.append(flux.DiskData(point(4), normal(), r, material()))
        else:
            c0 = rng.uniform(-5, 4, 3)
            ext = rng.uniform(0.1, 3.0, 3)
            shapes.append(flux.BoxData(tuple(float(x) for x in c0), tuple(float(x) for x in c0 + ext), material(),
                                       bool(rng.uniform() < 0.15)))
    if unit_normals:
        for s in shapes:
            if isinstance(s, (flux.PlaneData, flux.DiskData)):
                s.normal = _unit(s.normal)
    sd.shapes = shapes
    return sd


def add_meshes(flux, sd, rng):
    """One to three small triangle soups as test_random_meshes_against_the_oracle draws them, a Dielectric among their materials."""
    from flux_amd.scene import MeshData
    for _ in range(int(rng.integers(1, 4))):
        nv = int(rng.integers(3, 60))
        v = rng.uniform(-4, 4, (nv, 3))
        v[:, 1] = np.abs(v[:, 1]) * 0.5
        nt = int(rng.integers(1, 150))
        seen, tl = set(), []   # distinct triangles only; degenerate ones are kept (tests/test_gpu_fuzz.py says why)
        for tri in rng.integers(0, nv, (nt, 3)):
            key = frozenset(int(x) for x in tri)
            if len(key) == 3 and key in seen:
                continue
            seen.add(key)
            tl.append(tri)
        t = np.array(tl, dtype=np.uint32).reshape(-1, 3)
        k = int(rng.integers(0, 4))
        mat = (flux.MatteData((0.6, 0.5, 0.4), (0, 0, 0), 0.9) if k == 0 else
               flux.EmissiveData((0.3, 0.9, 0.4), 2.0) if k == 1 else
               flux.GlossyReflectiveData(0.7, (0.9, 0.9, 1.0), 50.0) if k == 2 else
               flux.DielectricData(1.5, (0.9, 1.0, 0.95)))
        sd.shapes.append(MeshData(v, t, mat))
    return sd


def non_unit_normal(flux, sd):
    """tests/test_gpu_fuzz.py has_non_unit_plane (abi.hip's rule, |n.n - 1| <= 4 eps) extended to disks, whose records follow the
    plane's rule."""
    return any(isinstance(s, (flux.PlaneData, flux.DiskData)) and abs(float(np.dot(s.normal, s.normal)) - 1.0) > 4.0 * 2.220446049250313e-16
               for s in sd.shapes)


def has_glass(flux, sd):
    return any(isinstance(s.material, flux.DielectricData) for s in sd.shapes)


def chunk_jobs(flux, base, chunk, mesh):
    """The chunk's jobs: (scene, sample_root, max_trace_depth, seed) for each of its CASES scenes.  Sample roots 2 and 3 are the
    static kernel's range, 8 and 9 the refill and split kernels' (81 samples leave a partial second batch); the first scene of an
    analytic chunk is 8 x 6 at 256 spp, the split kernel's default range."""
    rng = np.random.default_rng(RESEEDED.get((mesh, chunk), SEED_BASE[mesh] + chunk))
    jobs = []
    for case in range(CASES):
        big = case == 0 and not mesh
        sd = random_ext_scene(flux, base, rng, unit_normals=case % 4 != 3, frame=(8, 6) if big else None)
        if mesh:
            add_meshes(flux, sd, rng)
        n = int(rng.choice([2, 3, 8, 9, 8, 9]))   # (two draws in three at 64 spp or more: the refill and split kernels' range)
        D = int(rng.choice([2, 3, 5, 9]))
        seed = int(rng.integers(1, 1 << 30))
        jobs.append((sd, 16 if big else n, D, seed))
    return jobs


@functools.lru_cache(maxsize=None)
def chunk_references(chunk, mesh):
    """[(scene, n, D, seed, PathSpec with its frame made)] of a chunk: one reference per scene, made once for every test of the
    session that asks (tests/test_path_spec.py too) and never written to."""
    import flux_amd as flux
    base = flux.load_scene(os.path.join(SCENES, "demo1.yml"))
    out = []
    for sd, n, D, seed in chunk_jobs(flux, base, chunk, mesh):
        spec = path_spec.PathSpec(sd, n, D, seed)
        spec.frame().setflags(write=False)
        out.append((sd, n, D, seed, spec))
    return out


# ---- one run against the reference ------------------------------------------------------------------------------------------

def _explain(r, spec, got, want):
    """The worst pixel and, in it, the sample whose radiance differs most between the reference (PathSpec.sample) and the kernel
    (flux_debug_shade on the sample's primary ray with its set and index)."""
    with np.errstate(invalid="ignore"):
        diff = np.where(np.isfinite(got) & np.isfinite(want), np.abs(got - want), np.where(np.isfinite(got) == np.isfinite(want), 0.0, np.inf))
    row, col = np.unravel_index(np.argmax(diff.max(axis=2)), diff.shape[:2])
    o, d, sets = spec.primary
    worst, text = -1.0, ""
    for i in range(spec.N):
        rgb, hit, t = r.debug_shade(o[row, col, i][None, :], d[row, col, i][None, :], 1, int(sets[row, col]), i)
        ref = spec.sample(row, col, i)
        with np.errstate(invalid="ignore"):
            e = np.abs(rgb[0] - ref)
        e = float(np.nanmax(np.where(np.isnan(e), np.inf if np.isfinite(rgb[0]).all() != np.isfinite(ref).all() else 0.0, e)))
        if e > worst:
            worst, text = e, f"sample {i} (set {int(sets[row, col])}): reference {ref}, kernel {rgb[0]} first hit {int(hit[0])} t {float(t[0])!r}"
    return f"worst pixel ({row}, {col}): kernel {got[row, col]}, reference {want[row, col]}; its worst {text}"


def check_run(flux, r, spec, tag, unit, worst):
    """One render of the renderer as it is set up, against the reference: the ten statistics, the finite mask, the tolerances."""
    r.enable_stats(True)
    r.stats(reset=True)
    got = r.render_frame()
    st = r.stats()
    want = spec.frame()
    finite = np.isfinite(want)
    differing = [k for k in path_spec.STAT_NAMES if st[k] != spec.stats[k]]
    ok = not differing and np.array_equal(np.isfinite(got), finite) and (not unit or finite.all())
    err = np.abs(got[finite] - want[finite]) if finite.any() else np.zeros(1)
    if ok:
        ok = float(err.max()) < TOL and float(np.percentile(err, 99.9)) < TOL_TIGHT
    if not ok:
        first = f"{differing[0]}: kernel {st[differing[0]]}, reference {spec.stats[differing[0]]}" if differing else "statistics equal"
        why = f"{tag}: {first}; max |difference| {float(err.max()):.3e}, 99.9th percentile {float(np.percentile(err, 99.9)):.3e}; "
        raise AssertionError(why + _explain(r, spec, got, want))
    key = "STRICT" if r.launch_plan()["math"] == flux.MATH_STRICT else "FAST"
    worst[key] = max(worst.get(key, 0.0), float(err.max()))
    return got, st


def scene_lds(flux, sd):
    recs = sum(6 if isinstance(s, flux.BoxData) else 1 for s in sd.shapes)
    return recs * REC + sum(isinstance(s, flux.SphereData) for s in sd.shapes) * SPH


def hit_queue_candidate(flux, sd, n, unit):
    """The scenes the forced hit queue is tried on: FAST's own (unit normals), no glass, 64 spp or more."""
    return unit and not has_glass(flux, sd) and n * n >= 64


def forced_queue_fits(flux, sd, D):
    """launch_plan.cpp plan_hitq for a one-wave block, restated: the 6 LDS granules (7 680 B) hold the records, 96 B and the 66
    forced slots, and a path's bounce list (one record index a level) fits 32 bits.  The launch plan has the last word: every run
    below asserts that it agrees."""
    records = sum(6 if isinstance(s, flux.BoxData) else 1 for s in sd.shapes)
    bits = 1
    while (1 << bits) < records:
        bits += 1
    return 7680 - scene_lds(flux, sd) - 96 >= 66 * SLOT and bits * D <= 32


def _forced_queue(monkeypatch, take_at):
    switches.set_switches(monkeypatch, **switches.queue(None if take_at is None else (66, take_at)))


def _queue_is_on(flux, sd, plan):
    return plan["kernel"] == flux._lib.PLAN_SPLIT and plan["lds"] == plan["waves_per_pixel"] * 66 * SLOT + scene_lds(flux, sd)


def check_aov(flux, r, spec, tag):
    want = path_spec.aov_buffers(spec)
    for math in (flux.MATH_FAST, flux.MATH_STRICT):
        r.set_math(math)
        aov_spec.assert_close(r.render_aov(), want, f"{tag} math {math}")


@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_random_extension_scenes_against_the_path_reference(flux, monkeypatch, chunk):
    worst, queued = {}, 0
    for case, (sd, n, D, seed, spec) in enumerate(chunk_references(chunk, False)):
        cfg = flux.JobConfiguration(n, D, 50)
        unit = not non_unit_normal(flux, sd)
        tag0 = f"chunk {chunk} case {case} n {n} D {D} shapes {len(sd.shapes)}"
        _forced_queue(monkeypatch, None)
        with flux.Renderer(sd, cfg, seed=seed) as r:
            for math in (flux.MATH_FAST, flux.MATH_STRICT):
                r.set_math(math)
                assert r.launch_plan()["math"] == (math if unit else flux.MATH_STRICT), tag0
                for variant in (flux.KERNEL_STATIC, flux.KERNEL_REFILL, flux.KERNEL_SPLIT):
                    r.set_kernel(variant)
                    check_run(flux, r, spec, f"{tag0} math {math} kernel {variant}", unit, worst)
            if n == 8:
                r.set_kernel(flux.KERNEL_DEFAULT)
                check_aov(flux, r, spec, tag0)
        if hit_queue_candidate(flux, sd, n, unit):
            for take_at in (2, 1):
                _forced_queue(monkeypatch, take_at)   # before the context: its throughput table is sized at creation
                try:
                    with flux.Renderer(sd, cfg, seed=seed) as r:
                        r.set_kernel(flux.KERNEL_SPLIT)
                        assert _queue_is_on(flux, sd, r.launch_plan()) == forced_queue_fits(flux, sd, D), tag0
                        queued += forced_queue_fits(flux, sd, D)
                        check_run(flux, r, spec, f"{tag0} math {flux.MATH_FAST} kernel {flux.KERNEL_SPLIT} hit queue 66, take at {take_at}", unit, worst)
                finally:
                    _forced_queue(monkeypatch, None)
    print(f"ext fuzz chunk {chunk}: max |gpu - reference| " + ", ".join(f"{k} {v:.3e}" for k, v in sorted(worst.items())) +
          f"; {queued} runs with the forced hit queue on")


@pytest.mark.parametrize("chunk", range(MESH_CHUNKS))
def test_random_extension_scenes_beside_meshes(flux, chunk):
    """Boxes and disks scanned beside a mesh: the static kernel, the refill kernel and the default one (the BVH state machine from
    64 spp on), each over the 4-wide tree, brute force and the binary tree."""
    worst = {}
    for case, (sd, n, D, seed, spec) in enumerate(chunk_references(chunk, True)):
        unit = not non_unit_normal(flux, sd)
        tag0 = f"mesh chunk {chunk} case {case} n {n} D {D} shapes {len(sd.shapes)}"
        with flux.Renderer(sd, flux.JobConfiguration(n, D, 50), seed=seed) as r:
            for math in (flux.MATH_FAST, flux.MATH_STRICT):
                r.set_math(math)
                assert r.launch_plan()["math"] == (math if unit else flux.MATH_STRICT), tag0
                for variant in (flux.KERNEL_STATIC, flux.KERNEL_REFILL, flux.KERNEL_DEFAULT):
                    for trav in (flux._lib.TRAVERSE_BVH, flux._lib.TRAVERSE_BRUTE, flux._lib.TRAVERSE_BVH_BINARY):
                        r.set_kernel(variant)
                        r.set_traversal(trav)
                        check_run(flux, r, spec, f"{tag0} math {math} kernel {variant} traversal {trav}", unit, worst)
            if n == 8:
                r.set_kernel(flux.KERNEL_DEFAULT)
                r.set_traversal(flux._lib.TRAVERSE_BVH)
                check_aov(flux, r, spec, tag0)
    print(f"ext fuzz mesh chunk {chunk}: max |gpu - reference| " + ", ".join(f"{k} {v:.3e}" for k, v in sorted(worst.items())))


# ---- two and four waves a pixel -----------------------------------------------------------------------------------------------

PLAIN_DEPTH = 5


@functools.lru_cache(maxsize=None)
def plain_scene(k):
    """(scene, seed, its 64-spp PathSpec): the k-th 2 x 2 scene of the generator (a stream of its own) that has unit normals, no
    glass, a box and a disk, records that leave two waves a pixel room for the plan's own hit queue (2 000 B: 12 LDS granules a
    block less 96 B hold two queues of 96 slots beside them), hits for the queue to park -- at least 100 Matte or Glossy bounces
    in its 256 reference samples -- and no decision within 1e-9 of its threshold.  Chosen on the CPU, from the reference alone."""
    import flux_amd as flux
    base = flux.load_scene(os.path.join(SCENES, "demo1.yml"))
    rng = np.random.default_rng(8000)
    found = 0
    for _ in range(400):
        sd = random_ext_scene(flux, base, rng, True, frame=(2, 2))
        seed = int(rng.integers(1, 1 << 30))
        kinds = {type(s) for s in sd.shapes}
        if has_glass(flux, sd) or flux.BoxData not in kinds or flux.DiskData not in kinds or scene_lds(flux, sd) > 2000:
            continue
        spec = path_spec.PathSpec(sd, 8, PLAIN_DEPTH, seed)
        spec.frame()
        if spec.stats["matte_bounces"] + spec.stats["glossy_bounces"] >= 100 and spec.min_margin() > 1e-9:
            if found == k:
                return sd, seed, spec
            found += 1
    raise AssertionError("the generator drew no such scene")


@pytest.mark.parametrize("k,n", [(0, 91), (1, 128)])
def test_two_and_four_waves_a_pixel(flux, monkeypatch, k, n):
    """8 281 and 16 384 spp (two and four waves a pixel) with the plan's own hit queue.  The per-sample reference would take minutes
    there, so the link is transitive: at 64 spp the static kernel is held against the reference on the same scene (statistics
    equal, the tolerances of every run above), and at the large sample count the split kernel is held against the static kernel
    on the same job (statistics equal, frame within 1e-12: the same samples in another summation order)."""
    _forced_queue(monkeypatch, None)
    sd, seed, spec = plain_scene(k)
    D = PLAIN_DEPTH
    with flux.Renderer(sd, flux.JobConfiguration(8, D, 50), seed=seed) as r:
        r.set_kernel(flux.KERNEL_STATIC)
        check_run(flux, r, spec, f"plain scene {k} at 64 spp, static kernel", True, {})
    frames = {}
    with flux.Renderer(sd, flux.JobConfiguration(n, D, 50), seed=seed) as r:
        for variant in (flux.KERNEL_STATIC, flux.KERNEL_SPLIT):
            r.set_kernel(variant)
            r.enable_stats(True)
            r.stats(reset=True)
            frames[variant] = (r.render_frame(), r.stats(), r.launch_plan())
    a, sa, _ = frames[flux.KERNEL_STATIC]
    b, sb, plan = frames[flux.KERNEL_SPLIT]
    assert plan["kernel"] == flux._lib.PLAN_SPLIT and plan["waves_per_pixel"] == (2 if n == 91 else 4)
    slots, rest = divmod(plan["lds"] - scene_lds(flux, sd), plan["waves_per_pixel"] * SLOT)
    assert rest == 0 and slots >= 96, plan   # the hit queue, not the ray queue (5 120 B a wave is no multiple of 68)
    assert sa == sb, (sa, sb)
    print(f"plain scene {k}, {n * n} spp: max |split - static| = {np.abs(a - b).max():.3e}")
    assert np.abs(a - b).max() <= 1e-12
