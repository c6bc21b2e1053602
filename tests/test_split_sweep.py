"""The scenes of the split-kernel sweep (tests/split_sweep.py) are worth rendering -- judged on the CPU, by the oracle alone at the
jobs' full sample counts for the seven classes it knows and by tests/path_spec.py at 64 spp for the two with disks, boxes and glass
--, so that the GPU comparison of tests/test_gpu_split_sweep.py is not blind.  For every (scene, job):
  * Matte + glossy + specular bounces are at least 25 % of the samples: the hit queue has hits to park;
  * some path ends on an emitter, and the frame is not constant (max - min > 0.01);
  * some path is ended by the depth limit wherever the plan is expected to cut there;
  * the oracle counts misses in the scenes without an environment;
  * the path reference takes no decision within 1e-9 of its threshold (the two extension classes: what tests/test_gpu_ext_fuzz.py
    demands of its own scenes).
A draw that fails one is replaced by the next draw of its stream (split_sweep.DRAWS): every draw before the one in use must fail,
the one in use must pass, and a class may replace one draw in four at the most -- a class that needs more has a generator to fix.
For every class, over its twelve runs, every flag combination its row of the table expects occurs at least twice (the GPU test
asserts that the plan agrees), and the first plane of typ_axis lies on +x, -x, +y, -y, +z and -z once each.

The oracle on 8 threads, per (scene, job): 0.01 to 0.37 s, the 8 x 6 frames at 16384 spp the slowest; all of a class 0.6 to 1.6 s,
the two extension classes (the Python path reference at 64 spp) about 3 s each."""
import pytest

import split_sweep as sw


def _runs(flux, cls):
    out = []
    for index in range(6):
        sd, _ = sw.scene(cls, index)
        for root, depth in sw.jobs_of(index):
            out.append((index, root, depth, sd, sw.expected_flags(flux, sd, root, depth)))
    return out


@pytest.mark.parametrize("cls", sw.CLASSES)
def test_the_scenes_are_worth_rendering(flux, cls):
    replaced, seconds = 0, []
    for index in range(6):
        used = sw.DRAWS.get(cls, {}).get(index, 0)
        for draw in range(used):
            assert sw.failed_conditions(cls, index, draw), f"{cls} scene {index}: draw {draw} is worth rendering, yet draw {used} is in use"
        failed = sw.failed_conditions(cls, index, used)
        assert not failed, f"{cls} scene {index} draw {used}: {failed}"
        replaced += used
        if cls in sw.ORACLE_CLASSES:
            seconds += [sw.oracle_run(cls, index, used, root, depth)[2] for root, depth in sw.jobs_of(index)]
    print(f"{cls}: {replaced} of {replaced + 6} draws replaced" + (f"; the oracle took {min(seconds):.2f} to {max(seconds):.2f} s a case" if seconds else ""))
    assert 4 * replaced <= replaced + 6


def _count(runs, mask, value):
    return sum((flags & mask) == value for *_, flags in runs)


@pytest.mark.parametrize("cls", sw.CLASSES)
def test_every_expected_flag_combination_occurs(flux, cls):
    L = flux._lib
    runs = _runs(flux, cls)
    assert len(runs) == 12
    TYP, MAX32, HITQ, TABLE, CUT, UNI = (L.PLAN_FLAG_TYP, L.PLAN_FLAG_MAX32, L.PLAN_FLAG_HITQ, L.PLAN_FLAG_TPUT_TABLE,
                                         L.PLAN_FLAG_DEPTH_CUT, L.PLAN_FLAG_UNIFORM_A)
    AXIS, BITS, COPY = L.PLAN_FLAG_AXIS_MASK, L.PLAN_FLAG_HQ_BITS_MASK, L.PLAN_FLAG_COPY_MASK
    headline = TYP | MAX32 | HITQ | TABLE | CUT | UNI
    fast = 1 << L.PLAN_FLAG_COPY_SHIFT
    assert _count(runs, UNI, UNI) == 12
    assert _count(runs, COPY, 2 << L.PLAN_FLAG_COPY_SHIFT if cls == "glass" else fast) == 12
    if cls in ("typ_axis", "typ_no_axis", "records_17_30"):
        assert _count(runs, TYP | MAX32, TYP | MAX32) == 12
    else:
        assert _count(runs, TYP | AXIS, 0) == 12
    if cls == "typ_axis":
        for axis in (1, 2, 3):   # the whole headline combination on each axis, two scenes each
            assert _count(runs, headline | AXIS, headline | axis << L.PLAN_FLAG_AXIS_SHIFT) >= 2
        normals = [next(s.normal for s in sw.scene(cls, index)[0].shapes if isinstance(s, flux.PlaneData)) for index in range(6)]
        assert [str(n) for n in normals] == [str(a) for a in sw.AXES]   # (as text: the zeros' signs too)
    if cls == "typ_no_axis":
        assert _count(runs, headline | AXIS, headline) >= 2
        assert sum(not any(isinstance(s, flux.PlaneData) for s in sd.shapes) for *_, sd, _ in runs) >= 2   # no plane at all
    if cls == "records_17_30":
        five = 5 << L.PLAN_FLAG_HQ_BITS_SHIFT
        assert _count(runs, HITQ | TABLE | CUT | BITS, HITQ | five) >= 6    # depth 5: 25 bits, the hit queue; 48 MiB, no table, no cut
        assert _count(runs, HITQ | CUT | BITS, CUT) >= 2                    # depth 8: 40 bits, the ray queue
    if cls == "spheres_33_64":
        assert _count(runs, MAX32, 0) == 12
        assert _count(runs, HITQ, HITQ) >= 2 and _count(runs, HITQ | CUT, CUT) >= 2   # plan_hitq's rule: both outcomes
    if cls in ("no_env_shortcut", "beyond_the_guard", "five_exponents"):
        assert _count(runs, MAX32 | HITQ | TABLE | CUT, MAX32 | HITQ | TABLE | CUT) >= 2
    if cls == "five_exponents":
        for *_, sd, _ in runs:
            assert len({s.material.reflect_exponent for s in sd.shapes if isinstance(s.material, flux.GlossyReflectiveData)}) == 5
    if cls == "beyond_the_guard":
        for *_, sd, _ in runs:
            assert sum(max(abs(x) for x in s.center) > 1e3 or s.radius > 1e3 for s in sd.shapes if isinstance(s, flux.SphereData)) == 1
    if cls == "disks_and_boxes":
        assert _count(runs, MAX32 | HITQ, MAX32 | HITQ) >= 2 and _count(runs, HITQ | TABLE | CUT, HITQ | TABLE | CUT) >= 2
    if cls == "glass":
        assert _count(runs, HITQ | TABLE | CUT, CUT) == 12                  # a Dielectric keeps the ray queue, whose cut every job has
    if cls in ("disks_and_boxes", "glass"):
        for *_, sd, _ in runs:
            kinds = {type(s) for s in sd.shapes}
            assert flux.BoxData in kinds and flux.DiskData in kinds
            assert any(isinstance(s.material, flux.DielectricData) for s in sd.shapes) == (cls == "glass")


def test_normals_are_unit_and_cameras_inside(flux):
    """What every generator promises: unit plane and disk normals (the library's rule: |n.n - 1| <= 4 eps), the eye inside the
    environment where there is one, a lens radius of 0, 0.05 or 0.3 -- and all three occur."""
    lenses = set()
    for cls in sw.CLASSES:
        for index in range(6):
            sd, _ = sw.scene(cls, index)
            for s in sd.shapes:
                if isinstance(s, (flux.PlaneData, flux.DiskData)):
                    assert abs(sum(x * x for x in s.normal) - 1.0) <= 4.0 * 2.220446049250313e-16, (cls, index, s)
                if isinstance(s, flux.SphereData) and s.invert:
                    assert sum((e - c) ** 2 for e, c in zip(sd.camera_settings.eye, s.center)) < s.radius ** 2, (cls, index)
            lenses.add(sd.camera_data.lens_radius)
    assert lenses == {0.0, 0.05, 0.3}
