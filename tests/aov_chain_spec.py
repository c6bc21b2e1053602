"""The feature buffers at the first non-specular hit (include/flux_abi.h flux_render_aov_chain_rows) as numpy: the
reference the tests compare aov_chain_kernel against, and the test scenes.  No GPU.

It holds no second copy of the reference arithmetic.  The nearest hit is PathSpec._nearest; a Reflective bounce is oracle.sample_f
(the restatement's PerfectSpecular::sample_f) with scale (n.wi) / pdf; a Dielectric bounce is dielectric_spec.bounce with
u = hemi_sets[set][k - 1][i].z; a(m) is aov_spec.albedo, and the pixel's eight doubles are aov_spec._finish's.

The rule, per sample i of pixel (row, col) with set = row_perm(row)[col] % S and K the chain limit (max_chain, 0 = max_trace_depth):
the primary ray; at segment k the nearest hit; a miss ends the chain uncovered with albedo fold(background); a Reflective or
Dielectric hit with k < K bounces as the render does, tsum += t, k += 1; any other hit -- a delta material at k == K included --
ends the chain covered with albedo fold(a(m)) (the emissive facing test with this segment's direction), the hit's shading normal and
the depth term tsum + t.  fold(x) = (f * x) * s from the deepest bounce outward (STRICT's order; FAST multiplies the same factors front
to back, which the tests' tolerance covers).  GlossyReflective is not followed.  Nothing is clamped.

Every decision margin PathSpec records is recorded here by the same rules (MARGIN_NAMES; `glossy_flip` stays inf: no glossy lobe is
run)."""
import numpy as np

import aov_spec
import dielectric_spec
import path_spec
from oracle import oracle as oracle_mod

W, H, SEED, DEPTH = aov_spec.W, aov_spec.H, aov_spec.SEED, 5
DELTA = ("ReflectiveData", "DielectricData")


def _kind(x):
    return type(x).__name__


class Chain:
    """What chain_buffers found: `buffers` [H, W, 8]; per sample [H, W, N] `length` (segments traced), `covered`, `cut` (ended on a
    delta material at k == K) and `albedo` [H, W, N, 3] (folded); `margins`; the numbers of Dielectric `reflections` and
    `transmissions` and of `mirror_bounces`."""


def limit(spec, max_chain):
    if max_chain < 0 or max_chain > spec.D:
        raise ValueError(f"max_chain {max_chain} exceeds max_trace_depth {spec.D}")
    return spec.D if max_chain == 0 else max_chain


def _primary(spec):
    if getattr(spec, "primary", None) is None:
        spec.primary = spec.primary_rays()
    return spec.primary


def chain_buffers(spec, max_chain=0):
    """The chain feature buffers of a path_spec.PathSpec: a Chain."""
    with np.errstate(all="ignore"):
        return _chain_quiet(spec, limit(spec, max_chain))


def _chain_quiet(spec, K):
    o0, d0, sets = _primary(spec)
    Hh, Ww, N = o0.shape[:3]
    o, d = o0.reshape(-1, 3).copy(), d0.reshape(-1, 3).copy()
    m = len(o)
    set_of, idx_of = np.repeat(sets.ravel(), N), np.tile(np.arange(N), Hh * Ww)
    margins = {name: np.inf for name in path_spec.MARGIN_NAMES}
    end = np.zeros((m, 3))               # a(m) of the hit the chain ends at, or the background
    nrm, depth, covered = np.zeros((m, 3)), np.zeros(m), np.zeros(m, bool)
    length, cut, tsum = np.zeros(m, int), np.zeros(m, bool), np.zeros(m)
    bounces = []                         # per segment: (rays, f [j, 3], scale [j])
    out = Chain()
    out.reflections = out.transmissions = out.mirror_bounces = 0
    live = np.arange(m)
    for k in range(1, K + 1):
        if not len(live):
            break
        shape, t, n_hit, pt, _, tri = spec._nearest(o[live], d[live], margins)
        chosen = spec._materials(shape, o[live], d[live], tri, k)
        rays, fs, scales = [], [], []
        for j, ray in enumerate(live):
            length[ray] = k
            si = int(shape[j])
            if si < 0:
                end[ray] = spec.background
                continue
            mat, n, dr = chosen[j][0], n_hit[j], d[ray]
            if _kind(mat) in DELTA and k < K:
                if _kind(mat) == "DielectricData":
                    u = spec._hemi[set_of[ray], k - 1, idx_of[ray], 2]
                    refl, wi, F = dielectric_spec.bounce(n[None, :], dr[None, :], mat.refraction_index, np.array([u]))
                    spec._note(margins, "fresnel", abs(u - F[0]))
                    if refl[0]:
                        out.reflections += 1
                        f = np.ones(3)
                    else:
                        out.transmissions += 1
                        f = np.asarray(mat.transmit_color, dtype=np.float64)
                    wi, scale = wi[0], 1.0
                else:  # materials.rs:56-72
                    out.mirror_bounces += 1
                    mk, mp = chosen[j][1]
                    wi, pdf, f = oracle_mod.sample_f(mk, mp, n, dr * -1.0, spec._hemi[set_of[ray], k - 1, idx_of[ray]],
                                                     spec._pixel[set_of[ray], idx_of[ray]])
                    scale = path_spec._dot(n, wi) / np.float64(pdf)
                rays.append(ray)
                fs.append(f)
                scales.append(scale)
                tsum[ray] += t[j]
                o[ray], d[ray] = pt[j], wi
                continue
            if _kind(mat) == "EmissiveData":
                spec._note(margins, "emitter_facing",
                           abs(path_spec._dot(n * -1.0, dr)) / np.sqrt(path_spec._dot(n, n) * path_spec._dot(dr, dr)))
            end[ray] = aov_spec.albedo(mat, n, dr)
            nrm[ray], depth[ray], covered[ray] = n, tsum[ray] + t[j], True
            cut[ray] = _kind(mat) in DELTA
        live = np.array(rays, dtype=int)
        bounces.append((live, np.array(fs).reshape(-1, 3), np.array(scales)))
    alb = end
    for rays, f, scale in reversed(bounces):  # fold: (f * x) * s, the deepest bounce first
        if len(rays):
            alb[rays] = (f * alb[rays]) * scale[:, None]
    out.albedo = alb.reshape(Hh, Ww, N, 3)
    out.length, out.covered, out.cut = length.reshape(Hh, Ww, N), covered.reshape(Hh, Ww, N), cut.reshape(Hh, Ww, N)
    nrm, depth = nrm.reshape(Hh, Ww, N, 3), depth.reshape(Hh, Ww, N)
    asum, nsum, tsums, hits = np.zeros((Hh, Ww, 3)), np.zeros((Hh, Ww, 3)), np.zeros((Hh, Ww)), np.zeros((Hh, Ww))
    for i in range(N):  # in sample order, as aov_buffers sums
        asum = asum + out.albedo[:, :, i]
        c = out.covered[:, :, i]
        nsum = nsum + np.where(c[..., None], nrm[:, :, i], 0.0)
        tsums = tsums + np.where(c, depth[:, :, i], 0.0)
        hits = hits + c
    out.buffers = aov_spec._finish(asum, nsum, tsums, hits, N)
    out.margins = margins
    return out


# ---- the scenes: 16 x 12 ------------------------------------------------------------------------------------------------------

def mirror_scene(flux):
    """`open` with its Matte sphere Reflective, over its Reflective floor, and a Reflective wall behind it that leans over the sphere
    and the floor: chains between the three.  (An upright wall sends rays back past the camera to the floor's horizon, where a
    sphere 10^5 away is missed by a relative margin below 1e-9.)"""
    sd = aov_spec.open_scene(flux)
    sd.scene_name = "open_mirrors"
    sd.shapes[0].material = flux.ReflectiveData(0.9, (0.95, 0.9, 0.85))
    sd.shapes.append(flux.PlaneData((0.0, 0.0, 2.2), (0.0, -0.6, -0.8), flux.ReflectiveData(0.85, (0.9, 1.0, 0.9))))
    return sd


def mirror_emissive_scene(flux):
    """mirror_scene's geometry with every non-specular material Emissive: a path's radiance is fold(what its chain ends at).  Every
    colour, weight and power is a dyadic fraction of a few bits, none above 1: a sample's radiance is then an exact product, a
    pixel's sum of them is exact in whatever order it is formed -- the refill and split kernels add a pixel's 256 samples in other
    orders than the static kernel and the chain pass do (with colours like 0.9 their frames differ from the static kernel's, and
    from the chain albedo, in the last bit of some 80 of 471 values) --, and max_to_one leaves the frame alone."""
    sd = mirror_scene(flux)
    sd.scene_name = "open_mirrors_emissive"
    sd.background = (0.125, 0.25, 0.5)
    sd.shapes[0].material = flux.ReflectiveData(0.5, (1.0, 0.5, 0.75))
    sd.shapes[1].material = flux.EmissiveData((0.5, 0.75, 0.25), 1.0)
    sd.shapes[2].material = flux.EmissiveData((1.0, 0.5, 0.25), 1.0)
    sd.shapes[3].material = flux.ReflectiveData(0.75, (1.0, 1.0, 0.5))
    sd.shapes[4].material = flux.ReflectiveData(0.5, (0.5, 1.0, 1.0))
    return sd


def nonunit_mirror_scene(flux):
    """mirror_scene with the wall's normal of length 2: a FAST context runs it in STRICT."""
    sd = mirror_scene(flux)
    sd.scene_name = "open_mirrors_nonunit"
    sd.shapes[-1].normal = (0.0, -1.2, -1.6)
    return sd


def delta_free_scene(flux):
    """`open` with its Reflective floor Matte: nothing to follow."""
    sd = aov_spec.open_scene(flux)
    sd.scene_name = "open_delta_free"
    sd.shapes[-1].material = flux.MatteData((0.5, 0.5, 0.6), (0.0, 0.0, 0.0), 0.8)
    return sd


def mesh_mirror_scene(flux):
    """`open_mesh` with its quad Reflective too (the floor triangle already is): mirrors that are triangles."""
    sd = aov_spec.open_mesh_scene(flux)
    sd.scene_name = "open_mesh_mirrors"
    sd.shapes[0].material = flux.ReflectiveData(0.9, (0.95, 0.9, 0.85))
    sd.shapes[-2].material = flux.ReflectiveData(0.85, (0.9, 1.0, 0.9))
    return sd


def box_room_scene(flux):
    """scenes/box_room.yml at 16 x 12 with its glossy box Reflective and its sphere Dielectric, seen from beside the glass sphere
    with the mirror box behind it (at the file's camera the sphere covers a dozen pixels and too few chains pass it), and with the
    room opened: of the inverted box that encloses the scene only the floor is kept, as a plane of the room's material, under a
    sky of (0.1, 0.2, 0.3) -- samples miss, before and after glass and mirror bounces.  Box faces as chain vertices."""
    sd = shrunk(flux, "box_room", zoom=2.5, eye=(-7.0, 3.0, 0.0), look_at=(-1.5, 2.8, 2.5))
    sd.scene_name = "box_room_chain"
    room = sd.shapes[0]
    assert _kind(room) == "BoxData" and room.invert
    sd.shapes[0] = flux.PlaneData((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), room.material)
    sd.background = (0.1, 0.2, 0.3)
    for s in sd.shapes:
        if _kind(s.material) == "GlossyReflectiveData":
            s.material = (flux.ReflectiveData(0.9, (0.8, 0.9, 1.0)) if _kind(s) == "BoxData"
                          else flux.DielectricData(1.5, (0.9, 1.0, 0.95)))
    return sd


def glass_scene(flux):
    """scenes/glass.yml at 16 x 12, zoomed in by two so that its three glass spheres take a third of the samples, and opened: its
    environment sphere is dropped and the sky is (0.1, 0.2, 0.3), so that samples miss -- at once above the horizon and behind the
    glass (86 of them after a bounce) -- and the copy with the dielectric lobe folds the background and averages depth over covered samples only."""
    sd = shrunk(flux, "glass", zoom=2.0)
    env = sd.shapes[0]
    assert _kind(env) == "SphereData" and env.invert and env.radius == 100.0
    del sd.shapes[0]
    sd.background = (0.1, 0.2, 0.3)
    return sd


def shrunk(flux, name, zoom=1.0, eye=None, look_at=None):
    """scenes/<name>.yml at 16 x 12 with the same field of view, then the camera changes asked for."""
    import os
    from conftest import SCENES, small_scene
    sd = small_scene(flux.load_scene(os.path.join(SCENES, name + ".yml")), W, H)
    sd.camera_data.zoom_factor = sd.camera_data.zoom_factor * zoom
    if eye is not None:
        sd.camera_settings.eye = eye
    if look_at is not None:
        sd.camera_settings.look_at = look_at
    return sd


# name -> (scene builder, sample roots, has a Dielectric)
CASES = {
    "mirrors": (mirror_scene, (2, 3, 8, 10), False),
    "glass": (glass_scene, (4,), True),
    "box_room": (box_room_scene, (4,), True),
    "mesh": (mesh_mirror_scene, (8,), False),
    "nonunit": (nonunit_mirror_scene, (3,), False),
}


def case_spec(flux, name, root):
    return path_spec.PathSpec(CASES[name][0](flux), root, DEPTH, SEED)
