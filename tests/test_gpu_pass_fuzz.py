"""The two per-pixel passes on the extension fuzz's generated scenes (tests/test_gpu_ext_fuzz.py: 48 analytic and 16 mesh scenes of
8..12 x 6..9 pixels, sample roots 2, 3, 8, 9 and 16, depths 2 to 9, glass, boxes, disks and triangle soups, every fourth scene routed
to STRICT by its non-unit normals): the sample moments against moments_spec.from_samples of the scene's cached
PathSpec, and one adaptive run per scene (§5h) against adaptive_spec over the same PathSpec.  The references are those of the
render kernels' fuzz, made once per session; tests/test_pass_fuzz.py asserts on the CPU what the comparison rests on.

Tolerance: moments_spec.TOL in the forms of moments_spec.errors and adaptive_spec.errors, the pass map EQUAL.  Three scenes have
non-finite sample radiance (non-unit normals); there the finite mask must be the reference's in every channel and the bounds hold
wherever the reference is finite."""
import functools

import numpy as np
import pytest

import adaptive_spec as asp
import moments_spec as ms
from test_gpu_ext_fuzz import CASES, CHUNKS, MESH_CHUNKS, chunk_references, non_unit_normal

pytestmark = pytest.mark.gpu

# ---- the adaptive run of a scene ----------------------------------------------------------------------------------------------------
# max_passes 4 (every frame is at least 8 wide, so S >= 8), dilate 1, the other defaults, and for τ the first rung of LADDER at which
# the decision margin is >= 1e-9, the path margin >= 1e-10 and the pass map is not constant; 0.025 where no rung gives another map
# than a constant one (the margins must hold there too).  TAU pins search_tau's answer for the default chunks, [mesh][chunk][case]:
# the search runs the rule up to six times a scene, the pinned value once.  A chunk past the table (a longer soak) is searched.
LADDER = (0.8, 0.4, 0.2, 0.1, 0.05, 0.025)
ADAPTIVE = dict(max_passes=4, dilate=1)
TAU = {
    False: [(0.025, 0.4, 0.2, 0.2), (0.1, 0.4, 0.025, 0.8), (0.1, 0.05, 0.4, 0.025), (0.025, 0.4, 0.2, 0.2),
            (0.025, 0.8, 0.2, 0.05), (0.025, 0.1, 0.025, 0.025), (0.025, 0.4, 0.025, 0.2), (0.1, 0.025, 0.2, 0.025),
            (0.025, 0.025, 0.4, 0.025), (0.2, 0.2, 0.025, 0.8), (0.025, 0.025, 0.025, 0.05), (0.05, 0.05, 0.4, 0.025)],
    True: [(0.05, 0.4, 0.8, 0.8), (0.8, 0.4, 0.8, 0.025), (0.4, 0.025, 0.4, 0.8), (0.025, 0.025, 0.025, 0.8)],
}
# (mesh, chunk, case) of the default chunks whose sample radiance holds a NaN or an inf; (False, 7, 3) is NaN in every pixel
NON_FINITE = {(False, 2, 3), (False, 7, 3), (True, 0, 3)}
DECISION_MARGIN = 1e-9


def meets_the_margins(res):
    return res.decision_margin >= DECISION_MARGIN and res.path_margin >= ms.MIN_MARGIN


def search_tau(tp):
    for tau in LADDER:
        res = tp.run(**dict(asp.DEFAULTS, threshold=tau, **ADAPTIVE))
        if meets_the_margins(res) and len(np.unique(res.passes)) > 1:
            return tau
    return LADDER[-1]


@functools.lru_cache(maxsize=None)
def adaptive_reference(mesh, chunk, case):
    """(parameters, adaptive_spec.Result) of a scene's adaptive run, made once and never written to."""
    spec = chunk_references(chunk, mesh)[case][4]
    tp = asp.TracedPasses(spec)
    tau = TAU[mesh][chunk][case] if chunk < len(TAU[mesh]) else search_tau(tp)
    par = dict(asp.DEFAULTS, threshold=tau, **ADAPTIVE)
    res = tp.run(**par)
    res.moments.setflags(write=False)
    res.passes.setflags(write=False)
    return par, res


@functools.lru_cache(maxsize=None)
def moments_reference(mesh, chunk, case):
    spec = chunk_references(chunk, mesh)[case][4]
    mom = ms.from_samples(spec.sample_radiance)
    mom.setflags(write=False)
    return mom


# ---- one scene against its references ------------------------------------------------------------------------------------------------

def _worse(worst, key, err):
    for k, v in err.items():
        worst[(key, k)] = max(worst.get((key, k), 0.0), v)


def check_scene(flux, mesh, chunk, case, worst):
    L = flux._lib
    sd, n, D, seed, spec = chunk_references(chunk, mesh)[case]
    unit = not non_unit_normal(flux, sd)
    rad, want = spec.sample_radiance, moments_reference(mesh, chunk, case)
    par, awant = adaptive_reference(mesh, chunk, case)
    assert meets_the_margins(awant), (mesh, chunk, case)
    finite = bool(np.isfinite(want).all())
    assert finite or not unit
    tag0 = f"{'mesh ' if mesh else ''}chunk {chunk} case {case} n {n} D {D} shapes {len(sd.shapes)}"
    traversals = (("bvh", L.TRAVERSE_BVH), ("brute", L.TRAVERSE_BRUTE), ("binary", L.TRAVERSE_BVH_BINARY)) if mesh else ((None, None),)
    with flux.Renderer(sd, flux.JobConfiguration(n, D, 50), seed=seed) as r:
        r.set_kernel(flux.KERNEL_STATIC)
        for math in (flux.MATH_FAST, flux.MATH_STRICT):
            r.set_math(math)
            effective = r.launch_plan()["math"]
            assert effective == (math if unit else flux.MATH_STRICT), tag0
            name = "STRICT" if effective == flux.MATH_STRICT else "FAST"
            for trav_name, trav in traversals:
                if trav is not None:
                    r.set_traversal(trav)
                tag = f"{tag0} set_math {math} arithmetic {name} traversal {trav_name}"
                got = r.render_moments()
                (ms.assert_close if finite else ms.assert_close_where_finite)(got, want, rad, tag)
                with np.errstate(all="ignore"):
                    _worse(worst, "moments", ms.group_errors(got, want, ms.mean_lum(rad) ** 2, float(n * n), ms.max_to_one_factor(want)))
                frame = r.render_frame()
                differ = np.ascontiguousarray(got[..., ms.RGB]).view(np.uint64) != np.ascontiguousarray(frame).view(np.uint64)
                assert not differ.any(), (tag, "channels 0-2 differ from the static kernel's frame in", int(differ.sum()), "values, finite among them",
                                          int((differ & np.isfinite(frame)).sum()))
            if trav is not None:
                r.set_traversal(L.TRAVERSE_BVH)
            tag = f"{tag0} set_math {math} arithmetic {name}"
            amom, passes = r.render_adaptive(**par)
            info = r.last_adaptive_info
            if finite:
                asp.assert_close(amom, passes, awant, tag, n * n)
            else:
                asp.assert_close_where_finite(amom, passes, awant, tag, n * n)
            with np.errstate(all="ignore"):
                _worse(worst, "adaptive", ms.group_errors(amom, awant.moments, ms.lum(awant.moments[..., ms.MEAN]) ** 2,
                                                          n * n * awant.passes.astype(np.float64), ms.max_to_one_factor(awant.moments)))
            assert info["rounds"] == len(awant.active) and info["pixel_passes"] == int(awant.passes.sum()) == int(passes.sum()), tag
            assert info["pixels_at_max_passes"] == int(np.count_nonzero(awant.passes == par["max_passes"])), tag
            assert info["samples"] == n * n * int(passes.sum()), tag


def _report(label, worst):
    print(f"pass fuzz {label}: max error against the spec (rgb, mean absolute; var, s2 relative to ref + scale): " +
          "; ".join(f"{key} " + " ".join(f"{k} {worst.get((key, k), 0.0):.2e}" for k in ("rgb", "mean", "var", "s2")) for key in ("moments", "adaptive")))


@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_moments_and_adaptive_on_random_extension_scenes(flux, chunk):
    worst = {}
    for case in range(CASES):
        check_scene(flux, False, chunk, case, worst)
    _report(f"chunk {chunk}", worst)


@pytest.mark.parametrize("chunk", range(MESH_CHUNKS))
def test_moments_and_adaptive_beside_meshes(flux, chunk):
    """The moments in the three traversals, each against the spec and the static kernel's frame of that traversal."""
    worst = {}
    for case in range(CASES):
        check_scene(flux, True, chunk, case, worst)
    _report(f"mesh chunk {chunk}", worst)
