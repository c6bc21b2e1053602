"""The first-hit feature buffers (include/flux_abi.h flux_render_aov_rows) as Python: the reference the tests compare
the kernel against, the test scenes, and the image mapping of the command-line tool.  Plain functions.

For pixel (row, col) of a full context, with set = row_perm(row)[col] % S and N = sample_root²: for every i < N the primary ray the
render kernels build for (row, col, set, i) (trace.rs:71-80) and its first hit by Scene::hit.  Per sample: albedo a(material) on a
hit and the background on a miss; the shading normal on a hit and 0 on a miss; t and a count of one on a hit.  The pixel's 8 doubles:
mean albedo over N, mean normal over N, depth = sum of t / hits (0 without a hit), coverage = hits / N.  Nothing is clamped."""
import copy
import types

import numpy as np

import box_spec

CHANNELS = 8
ALBEDO, NORMAL, DEPTH, COVERAGE = slice(0, 3), slice(3, 6), 6, 7
SEED = 7
W, H = 16, 12


# ---- a(m) -------------------------------------------------------------------------------------------------------------------

def albedo(material, normal, direction):
    """a(m) of a hit with shading normal `normal` by a ray of direction `direction`."""
    m = material
    kind = type(m).__name__
    if kind == "MatteData":
        return m.diffuse_coefficient * np.asarray(m.diffuse_color, dtype=np.float64)
    if kind in ("ReflectiveData", "GlossyReflectiveData"):
        return m.reflect_amount * np.asarray(m.reflect_color, dtype=np.float64)
    if kind == "DielectricData":
        return np.asarray(m.transmit_color, dtype=np.float64)
    if kind == "EmissiveData":  # materials.rs:44: the side it emits to
        if -float(np.dot(normal, direction)) > 0.0:
            return m.power * np.asarray(m.color, dtype=np.float64)
        return np.zeros(3)
    raise TypeError(kind)


# ---- the scenes -------------------------------------------------------------------------------------------------------------

def _open_parts(flux):
    spheres = [
        flux.SphereData((0.0, 0.0, 0.0), 1.0, flux.MatteData((0.8, 0.6, 0.4), (0.0, 0.0, 0.0), 0.9), False),
        flux.SphereData((1.2, 0.3, 0.5), 0.6, flux.GlossyReflectiveData(0.7, (0.9, 0.9, 0.5), 50.0), False),
        flux.SphereData((-1.1, 0.9, -0.4), 0.5, flux.EmissiveData((1.0, 0.9, 0.8), 3.0), False),
    ]
    plane = flux.PlaneData((0.0, -1.0, 0.0), (0.0, 1.0, 0.0), flux.ReflectiveData(0.8, (0.9, 0.9, 0.9)))
    return spheres, plane


def _scene(flux, name, shapes):
    return flux.SceneData(name, flux.OutputSettings(W, H, 0.25), (0.1, 0.2, 0.3), shapes,
                          flux.CameraSettings((0.0, 1.0, -6.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)), flux.CameraData(1.0, 8.0, 6.0, 0.15))


def open_scene(flux):
    """`open`: three spheres over a plane, the background visible above the horizon."""
    spheres, plane = _open_parts(flux)
    return _scene(flux, "open", spheres + [plane])


def open_mesh_scene(flux):
    """`open_mesh`: `open` with the plane replaced by a two-triangle quad and a one-triangle mesh."""
    from flux_amd.scene import MeshData
    spheres, _ = _open_parts(flux)
    quad = MeshData(np.array([(-2, -0.5, 1.5), (2, -0.5, 1.5), (2, 2, 2.5), (-2, 2, 2.5)], dtype=np.float64),
                    np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint32), flux.MatteData((0.2, 0.7, 0.3), (0.0, 0.0, 0.0), 0.8))
    tri = MeshData(np.array([(-3, -1, -1), (3, -1, -1), (0, -1, 4)], dtype=np.float64), np.array([[0, 1, 2]], dtype=np.uint32),
                   flux.ReflectiveData(0.8, (0.9, 0.9, 0.9)))
    return _scene(flux, "open_mesh", spheres + [quad, tri])


def open_emissive_scene(flux):
    """`open` with every material replaced by Emissive(c, 1.0), c <= 1: at max_trace_depth 1 the render IS the albedo buffer."""
    sd = open_scene(flux)
    colors = [(0.8, 0.6, 0.4), (0.9, 0.9, 0.5), (1.0, 0.9, 0.8), (0.9, 0.9, 0.9)]
    for s, c in zip(sd.shapes, colors):
        s.material = flux.EmissiveData(c, 1.0)
    return sd


# ---- the reference ------------------------------------------------------------------------------------------------------------

def _finish(alb, nrm, tsum, hits, N):
    out = np.zeros(alb.shape[:2] + (CHANNELS,))
    out[..., ALBEDO] = alb / N
    out[..., NORMAL] = nrm / N
    with np.errstate(invalid="ignore", divide="ignore"):
        out[..., DEPTH] = np.where(hits > 0, tsum / np.maximum(hits, 1), 0.0)
    out[..., COVERAGE] = hits / N
    return out


def _facts(hits, N):
    return {"misses": int(hits.size * N - hits.sum()), "samples": int(hits.size * N),
            "partly_covered": int(np.count_nonzero((hits > 0) & (hits < N)))}


def _materials_in_hit_order(sd):
    """The material of every hit index of the restatement: the analytic shapes in order, then every mesh's triangles."""
    mats = [s.material for s in sd.shapes if type(s).__name__ != "MeshData"]
    for s in sd.shapes:
        if type(s).__name__ == "MeshData":
            mats += [s.material] * len(np.asarray(s.triangles).reshape(-1, 3))
    return mats


def reference(oracle_mod, sd, root, seed=SEED):
    """(buffers [H, W, 8], facts) from the CPU restatement: its row permutation, primary rays, first hits and normals."""
    cfg = types.SimpleNamespace(sample_root=root, max_trace_depth=1, rows_per_work_unit=50)
    O = oracle_mod.Oracle(sd, cfg, seed=seed)
    try:
        w, h, N = O.width, O.height, root * root
        mats = _materials_in_hit_order(sd)
        bg = np.asarray(sd.background, dtype=np.float64)
        alb, nrm = np.zeros((h, w, 3)), np.zeros((h, w, 3))
        tsum, hits = np.zeros((h, w)), np.zeros((h, w))
        for row in range(h):
            perm = O.row_perm(row)
            for col in range(w):
                s = int(perm[col]) % w
                for i in range(N):
                    o, d = O.primary_ray(row, col, s, i)
                    idx, t, n, _ = O.scene_hit(o, d)
                    if idx < 0:
                        alb[row, col] += bg
                        continue
                    alb[row, col] += albedo(mats[idx], n, d)
                    nrm[row, col] += n
                    tsum[row, col] += t
                    hits[row, col] += 1
    finally:
        O.close()
    return _finish(alb, nrm, tsum, hits, N), _facts(hits, N)


def primary_rays(oracle_mod, sd, root, seed=SEED):
    """(o, d) [H, W, N, 3] of the restatement's camera alone (an Oracle of the same camera without shapes)."""
    bare = copy.copy(sd)
    bare.shapes = []
    cfg = types.SimpleNamespace(sample_root=root, max_trace_depth=1, rows_per_work_unit=50)
    O = oracle_mod.Oracle(bare, cfg, seed=seed)
    try:
        w, h, N = O.width, O.height, root * root
        o, d = np.empty((h, w, N, 3)), np.empty((h, w, N, 3))
        for row in range(h):
            perm = O.row_perm(row)
            for col in range(w):
                s = int(perm[col]) % w
                for i in range(N):
                    o[row, col, i], d[row, col, i] = O.primary_ray(row, col, s, i)
    finally:
        O.close()
    return o, d


def reference_debug_shade(flux, oracle_mod, sd, root, math_mode, seed=SEED):
    """(buffers, facts, first-hit shape indices [H, W, N]) for a scene the restatement rejects (Disk, Box, Dielectric): the
    restatement's rays, first hit and t from Renderer.debug_shade, normals from the shape's own rule."""
    o, d = primary_rays(oracle_mod, sd, root, seed)
    h, w, N, _ = o.shape
    of, df = o.reshape(-1, 3), d.reshape(-1, 3)
    with flux.Renderer(sd, flux.JobConfiguration(root, 1, 50), seed=seed) as r:
        r.set_math(math_mode)
        _, hit, t = r.debug_shade(of, df, 1, 0, 0)
    bg = np.asarray(sd.background, dtype=np.float64)
    alb, nrm = np.zeros((len(of), 3)), np.zeros((len(of), 3))
    tt, hh = np.zeros(len(of)), np.zeros(len(of))
    for k in range(len(of)):
        idx = int(hit[k])
        if idx < 0:
            alb[k] = bg
            continue
        s = sd.shapes[idx]
        kind = type(s).__name__
        if kind == "SphereData":
            q = of[k] + t[k] * df[k]
            n = (q - np.asarray(s.center, dtype=np.float64)) * (-1.0 if s.invert else 1.0) / s.radius
        elif kind == "BoxData":
            ok, _, nb, _, _ = box_spec.box_hit(s.corner0, s.corner1, of[k], df[k], invert=s.invert)
            assert ok[0], (idx, k)
            n = nb[0]
        else:  # Plane, Disk: as stored
            n = np.asarray(s.normal, dtype=np.float64)
        alb[k] = albedo(s.material, n, df[k])
        nrm[k] = n
        tt[k] = t[k]
        hh[k] = 1.0
    hits = hh.reshape(h, w, N).sum(axis=2)
    out = _finish(alb.reshape(h, w, N, 3).sum(axis=2), nrm.reshape(h, w, N, 3).sum(axis=2), tt.reshape(h, w, N).sum(axis=2), hits, N)
    return out, _facts(hits, N), hit.reshape(h, w, N)


# ---- comparison ---------------------------------------------------------------------------------------------------------------

TOL = 1e-9


def channel_errors(got, want):
    """The largest |difference| per channel; the depth channel relative to max(1, depth)."""
    diff = np.abs(np.asarray(got) - np.asarray(want))
    with np.errstate(invalid="ignore"):
        both_inf = np.isinf(got[..., DEPTH]) & (got[..., DEPTH] == want[..., DEPTH])
        diff[..., DEPTH] = np.where(both_inf, 0.0, diff[..., DEPTH] / np.maximum(1.0, np.abs(want[..., DEPTH])))
    return diff.reshape(-1, CHANNELS).max(axis=0)


def assert_close(got, want, label):
    """|Δ| <= 1e-9 on channels 0-5 and 7, |Δ| <= 1e-9 max(1, depth) on depth, every pixel; prints the figures first."""
    err = channel_errors(got, want)
    print(f"aov {label}: max |gpu - spec| per channel = " + " ".join(f"{e:.2e}" for e in err))
    assert got.shape == want.shape
    assert np.all(err <= TOL), (label, err)


# ---- the command-line tool's images (flux_amd/host/flux_host.hpp aov_image) -----------------------------------------------------

def aov_image(aov, kind):
    """RGB in [0, 1] of one channel group: 'albedo' min(1, x); 'normal' 0.5 + 0.5 n/|n| (zero vector: 0.5); 'depth' grey
    coverage (1 - t / t_max), t_max the largest finite depth of the frame (1 if none), non-finite depth 0; 'coverage' grey."""
    aov = np.asarray(aov, dtype=np.float64)
    if kind == "albedo":
        return np.minimum(1.0, aov[..., ALBEDO])
    if kind == "normal":
        n = aov[..., NORMAL]
        ln = np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2])[..., None]
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(ln > 0.0, 0.5 + 0.5 * (n / ln), 0.5)
    if kind == "depth":
        t = aov[..., DEPTH]
        fin = np.isfinite(t)
        t_max = float(t[fin].max()) if fin.any() else 0.0
        if not t_max > 0.0:
            t_max = 1.0
        with np.errstate(invalid="ignore"):
            g = np.where(fin, aov[..., COVERAGE] * (1.0 - t / t_max), 0.0)
        return np.repeat(g[..., None], 3, axis=2)
    if kind == "coverage":
        return np.repeat(aov[..., COVERAGE][..., None], 3, axis=2)
    raise ValueError(kind)
