"""The split kernel's TYP instantiations take the first scan plane's test as num = p_a - o_a, den = d_a where the host has found the
plane's stored normal on an axis (RenderParams::plane_axis, flux_amd/csrc/flux_plane_axis.h), in every wave whose vote admits it.
FLUX_PLANE_AXIS=0 builds the context without the axis: both scans then form the dot products in full.  The two may not differ in a
single bit: every scene here is rendered both ways with the hit-queue kernel (the plan's own choice at this sample count), with the
ray-queue kernel (FLUX_SPLIT_HITQ_CAP=0) and with phase A's general shading step (FLUX_SPLIT_UNIFORM_A=0) -- np.array_equal, equal path
statistics -- and the frame with the axis has the oracle's path statistics and its image to 1e-4 (the tolerance of
tests/test_gpu_lobe_frames.py).

8 x 6 pixels at sample root 128 (16384 spp: four waves a pixel and the hit queue, as the benchmark's headline), depth limit 5.  The
scenes: demo2 with scene and camera turned so that the floor's normal is +x, -x, +y (demo2 itself), -y, +z, -z -- a turn by right angles
is a signed permutation of the coordinates, so the stored normal stays exact, with zeros of either sign; a floor tilted about z (a unit
normal on no axis: classified "none", the switch must change nothing); the floor followed by a tilted back wall (the axis-aligned plane
first: the reduced form runs, the wall goes through the later-planes loop) and the wall followed by the floor (the first plane is on no
axis).  CPU side: tests/test_plane_axis.py."""
import copy

import numpy as np
import pytest

import split_checks as sc
from conftest import small_scene
from split_checks import TOL_ORACLE
from switches import switches  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu

N, DEPTH, SEED = 128, 5, 4
TURNED = {"floor_normal_" + name: turn for name, turn in sc.TURNS.items()}
CASES = list(TURNED) + ["tilted_floor", "floor_then_tilted_wall", "tilted_wall_then_floor"]
KERNELS = {"hit_queue": {}, "ray_queue": {"FLUX_SPLIT_HITQ_CAP": "0"}, "general_phase_a": {"FLUX_SPLIT_UNIFORM_A": "0"}}


def _cases(flux, demo2):
    base = small_scene(demo2, 8, 6)
    floor = next(s for s in base.shapes if isinstance(s, flux.PlaneData))
    others = [s for s in base.shapes if s is not floor]
    assert tuple(floor.normal) == (0.0, 1.0, 0.0) and sum(isinstance(s, flux.PlaneData) for s in base.shapes) == 1

    def scene(shapes):
        sd = copy.deepcopy(base)
        sd.shapes = copy.deepcopy(shapes)
        return sd

    cases = {name: sc.turned(flux, base, turn) for name, turn in TURNED.items()}
    for name, axis in (("plus_y", (0.0, 1.0, 0.0)), ("minus_y", (0.0, -1.0, 0.0)), ("plus_x", (1.0, 0.0, 0.0)), ("minus_x", (-1.0, 0.0, 0.0)),
                       ("plus_z", (0.0, 0.0, 1.0)), ("minus_z", (0.0, 0.0, -1.0))):
        plane = next(s for s in cases["floor_normal_" + name].shapes if isinstance(s, flux.PlaneData))
        assert tuple(plane.normal) == axis  # (compares equal: a zero of either sign)
    cases["tilted_floor"] = scene(others + [flux.PlaneData(floor.point, (0.6, 0.8, 0.0), floor.material)])
    # a wall behind the spheres that leans towards the eye: a unit normal on no axis
    wall = flux.PlaneData((0.0, 0.0, 12.0), (0.0, 0.6, -0.8), floor.material)
    cases["floor_then_tilted_wall"] = scene(others + [floor, wall])
    cases["tilted_wall_then_floor"] = scene(others + [wall, floor])
    assert sorted(cases) == sorted(CASES)
    return cases


_oracle = {}   # the oracle's frame and statistics of a case: read by every kernel


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("case", CASES)
def test_reduced_plane_test_changes_no_bit(flux, oracle_mod, demo2, switches, case, kernel):
    sd = _cases(flux, demo2)[case]
    want, o_stats = sc.references(_oracle, case, flux, oracle_mod, sd, N, DEPTH, SEED, kernels=())
    switches(**KERNELS[kernel])
    # (plain: the frame of the instantiation without statistics, the benchmark's, before the one that counts)
    got, gs, plan, _, plain = sc.render(flux, sd, N, DEPTH, SEED, flux.KERNEL_SPLIT, plain=True)
    switches(FLUX_PLANE_AXIS="0", **KERNELS[kernel])
    general, es, plan_general, _, plain_general = sc.render(flux, sd, N, DEPTH, SEED, flux.KERNEL_SPLIT, plain=True)
    switches(FLUX_SPLIT_HITQ_CAP="0")
    ray_queue_lds = sc.render(flux, sd, N, DEPTH, SEED, flux.KERNEL_SPLIT, plain=True).plan["lds"]
    switches()
    # which kernel ran: the split kernel, four waves a pixel; with the hit queue unless the case takes it away (the ray queue's 64
    # entries a wave are the smaller allocation)
    assert plan == plan_general
    assert plan["kernel"] == flux._lib.PLAN_SPLIT and plan["waves_per_pixel"] == 4
    assert (plan["lds"] == ray_queue_lds) == (kernel == "ray_queue")
    err = float(np.abs(got - want).max())
    print(f"{case} {kernel}: |split - oracle| {err:.3e}  bits equal to the general form: {np.array_equal(got, general)}  "
          f"segments {gs['segments']}")
    assert np.array_equal(got, general)
    assert np.array_equal(plain, plain_general)
    assert gs == es, (gs, es)
    assert {k: gs[k] for k in o_stats} == o_stats
    assert err < TOL_ORACLE
