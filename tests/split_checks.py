"""What the suites of the split kernel (tests/test_gpu_*.py around render_body.inc render_split_kernel) share: one render with
statistics, the oracle's run, the references of a case made once, the two frame comparisons and their tolerances, the LDS layout
numbers the plan's bytes are checked against, the hit queue's override pairs and demo2's right-angle turns.  Plain functions, as
tests/extension_checks.py: no fixtures -- each test states its own scenes, switches and assertions, and takes the `switches`
fixture from tests/switches.py."""
import collections
import copy
import os

import numpy as np

import switches

TOL_ORACLE = 1e-4    # a FAST frame against the CPU oracle's (tests/test_gpu_parity.py)
TOL_ORDER = 1e-12    # the same samples summed in another order: the split kernel against refill, static, or itself under a switch

# bytes in LDS, as the launch plan reserves them (launch_plan.cpp split_scene_lds, plan_hitq)
REC = 96             # sizeof(DevHitRec), flux_device.h: a record per shape, six per box
SPH = 32             # sizeof(DevScanSphere), flux_device.h
SLOT = 68            # flux_plan.h kHitQBytesPerSlot: a hit-queue slot
RAY_QUEUE = 5120     # flux_plan.h kQueueBytesPerWave: a wave's 64-entry ray queue

# (C, H) for FLUX_SPLIT_HITQ_CAP / FLUX_SPLIT_HITQ_TAKE_AT (switches.queue), the one-wave hit queues a default plan does not choose
# (launch_plan.cpp plan_hitq: one wave a pixel has 6 granules of 1280 B less the scene and 96 B of partial sums, and takes H >= 32):
Q_LARGEST = (86, 22)   # the most slots a one-wave block holds beside demo2's records; H = C - 64, the room left after a pass's 64 hits
Q_SMALLEST = (66, 1)   # the smallest pool the plan accepts (64 + H, even), taken in one-hit batches
QUEUES = [None, Q_LARGEST, Q_SMALLEST]   # None: the plan's own queue

TURNS = {  # name -> where (x, y, z) goes; each takes demo2's floor normal (0, 1, 0) to the axis in the name
    "plus_y": lambda v: (v[0], v[1], v[2]),
    "minus_y": lambda v: (-v[0], -v[1], v[2]),
    "plus_x": lambda v: (v[1], -v[0], v[2]),
    "minus_x": lambda v: (-v[1], v[0], v[2]),
    "plus_z": lambda v: (v[0], -v[2], v[1]),
    "minus_z": lambda v: (v[0], v[2], -v[1]),
}

Run = collections.namedtuple("Run", "frame stats plan device_bytes plain")
SAME = object()   # references(oracle_sd=SAME): the oracle renders the scene itself


def turned(flux, sd, turn):
    """A scene of spheres and planes, camera included, turned by one of TURNS"""
    sd = copy.deepcopy(sd)
    for s in sd.shapes:
        if isinstance(s, flux.SphereData):
            s.center = turn(s.center)
        else:
            assert isinstance(s, flux.PlaneData)
            s.point, s.normal = turn(s.point), turn(s.normal)
    cs = sd.camera_settings
    cs.eye, cs.look_at, cs.up = turn(cs.eye), turn(cs.look_at), turn(cs.up)
    return sd


def scene_lds(flux, sd):
    """The split kernel's scene copy in LDS"""
    records = sum(6 if isinstance(s, flux.BoxData) else 1 for s in sd.shapes)  # a box: one record per face
    return records * REC + sum(isinstance(s, flux.SphereData) for s in sd.shapes) * SPH


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def distance(a, b):
    """max |a - b| over the pixels finite in both; the finiteness patterns must be equal"""
    fa, fb = np.isfinite(a), np.isfinite(b)
    assert np.array_equal(fa, fb), "finiteness patterns differ"
    return float(np.abs(a[fa] - b[fa]).max()) if fa.any() else 0.0


def with_stats(flux, r, kernel=None):
    """(frame, statistics) of an open renderer, with `kernel` if one is given"""
    if kernel is not None:
        r.set_kernel(kernel)
    r.enable_stats(True)
    r.stats(reset=True)
    frame = r.render_frame()
    return frame, r.stats()


def split_run(flux, r, flags=True):
    """The split kernel of the context as it stands: frame without statistics, frame with, statistics, plan"""
    r.set_kernel(flux.KERNEL_SPLIT)
    r.enable_stats(False)
    plain = r.render_frame()
    frame, stats = with_stats(flux, r)
    return plain, frame, stats, r.launch_plan(flags=flags)


def render(flux, sd, root, depth, seed, kernel=None, plain=False):
    """One frame with statistics from a context of its own; `plain`: the frame of the instantiation without statistics (the
    benchmark's) first."""
    with flux.Renderer(sd, flux.JobConfiguration(root, depth, 50), seed=seed) as r:
        if kernel is not None:
            r.set_kernel(kernel)
        first = r.render_frame() if plain else None
        frame, stats = with_stats(flux, r)
        return Run(frame, stats, r.launch_plan(), r.device_bytes(), first)


def oracle_run(flux, oracle_mod, sd, root, depth, seed, threads=8):
    """(frame, statistics) of the CPU oracle; the frame is read-only"""
    o = oracle_mod.Oracle(sd, flux.JobConfiguration(root, depth, 50), seed=seed)
    try:
        o.stats(reset=True)
        frame = o.render_frame(threads=threads)
        frame.setflags(write=False)
        return frame, o.stats()
    finally:
        o.close()


def references(cache, key, flux, oracle_mod, sd, root, depth, seed, oracle_sd=SAME, kernels=("REFILL", "STATIC")):
    """(the oracle's frame, its statistics, one Run per kernel of `kernels`) of a job, made once per `key` in the caller's `cache`
    with no library switch set, every array read-only.  oracle_sd: the scene the oracle renders where it does not know `sd`'s
    shapes; None: no oracle (None, None)."""
    if key not in cache:
        assert not any(name in os.environ for name in switches.NAMES), "a reference made under a switch"
        want = (None, None)
        if oracle_sd is not None:
            want = oracle_run(flux, oracle_mod, sd if oracle_sd is SAME else oracle_sd, root, depth, seed)
        runs = tuple(render(flux, sd, root, depth, seed, getattr(flux, "KERNEL_" + k)) for k in kernels)
        for run in runs:
            run.frame.setflags(write=False)
        cache[key] = want + runs
    return cache[key]
