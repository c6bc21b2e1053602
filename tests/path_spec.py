"""A full-path reference for scenes with the extensions (Disk, Box, Dielectric: DESIGN.md §5b, §5c, §5d), which the frozen CPU
restatement (oracle/) rejects.  Plain Python and numpy, no GPU.  It holds no second copy of the arithmetic of the reference's own
shapes and materials: those are the restatement's entry points, called per ray.

  from the restatement   Oracle.primary_ray, row_perm, hemi_sets, pixel_sets; Oracle.scene_hit on a context that holds only the
                         scene's spheres, planes and meshes (a Dielectric on one of them is replaced by a Matte there: only the
                         geometry is asked for); oracle.sample_f, material_params, max_to_one
  from the numpy specs   box_spec.box_hit, dielectric_spec.bounce, and the disk rule of DESIGN.md §5b (`disk_hit` below)
  here                   the nearest hit over both groups, and Scene::shade / path_shade (flux_oracle.c:632-692) turned inside out:
                         a path is followed forwards, each bounce leaving its (f, n.wi / pdf), and the radiance of its end is folded
                         back through them from the deepest bounce, `(f * child) * scale` -- the products the recursion forms, in
                         its order.  The rays of one depth are taken together, so that the numpy specs see arrays; every ray's
                         decisions are its own.

Nearest hit: an equal t goes to the lower YAML index among the analytic shapes; triangles follow all shapes (they win only with a
strictly smaller t).  The hit point is the restatement's for its shapes and o + t d for the extensions.

Besides the result, `margins` holds the smallest margin of every kind of decision taken (see MARGIN_NAMES): a comparison of a kernel's
path statistics with this reference's is a fair demand only where no decision sits at rounding level.  The sphere and plane
quantities among them are computed in numpy beside the restatement's call and serve the margins alone, never a decision.
`classes` counts the segments per (shape kind, material) and a few more classes, for the coverage conditions of the fuzz."""
import collections
import copy
import types

import numpy as np

import box_spec
import dielectric_spec
from flux_amd.scene import MatteData
from oracle import oracle as oracle_mod

T_MIN = box_spec.T_MIN
STAT_NAMES = ("samples", "segments", "matte_bounces", "glossy_bounces", "specular_bounces", "emissive_hits", "misses",
              "depth_exhausted", "dielectric_reflections", "dielectric_transmissions")
MARGIN_NAMES = ("box_rounding_level",  # the pairs box_spec.rounding_level compares, relative: t0 | t1 ~ T_MIN, t0 ~ t1, the two largest tmin, the two smallest tmax
                "disk_rim",            # | |q - c|^2 - r^2 | / r^2
                "t_min",               # |t - T_MIN| / T_MIN of every candidate root of a sphere, plane or disk
                "nearest_gap",         # (t_second - t_first) / t_first of the two nearest candidates
                "sphere_discriminant",  # |disc| / b^2
                "fresnel",             # |u - F|
                "emitter_facing",      # |n.d| / (|n| |d|) at an Emissive hit
                "glossy_flip")         # |n.wi0| / (|n| |wi0|) of the glossy lobe's unmirrored direction
_STAND_IN = MatteData((0.5, 0.5, 0.5), (0.0, 0.0, 0.0), 1.0)


def _kind(x):
    return type(x).__name__


def _dot(a, b):
    """v3_dot: (x x' + y y') + z z', on single vectors or on rows."""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def disk_hit(center, normal, radius, o, d):
    """DESIGN.md §5b on rays o, d [m, 3]: (hit [m], t [m], dist2 [m]).  t = ((c - o).n) / (d.n) with Plane::hit's operands in its
    order; a hit iff t is finite, t > T_MIN and |o + t d - c|^2 <= r^2."""
    c, n = np.asarray(center, dtype=np.float64), np.asarray(normal, dtype=np.float64)
    t = _dot(c - o, n[None, :]) / _dot(d, n[None, :])
    q = o + t[:, None] * d
    dist2 = _dot(q - c, q - c)
    return np.isfinite(t) & (t > T_MIN) & (dist2 <= radius * radius), t, dist2


def box_margin(t0, t1, tmin, tmax):
    """The smallest relative distance among the pairs box_spec.rounding_level compares, per ray: rounding_level(eps) is
    `box_margin <= eps` (tests/test_path_spec.py holds the two against each other)."""
    def rel(x, y):
        ok = np.isfinite(x) & np.isfinite(y)
        return np.where(ok, np.abs(x - y) / np.maximum(np.maximum(np.abs(x), np.abs(y)), 1e-300), np.inf)
    lo = np.sort(np.where(np.isnan(tmin), -np.inf, tmin), axis=1)
    hi = np.sort(np.where(np.isnan(tmax), np.inf, tmax), axis=1)
    tm = np.full_like(t0, T_MIN)
    return np.minimum.reduce([rel(t0, tm), rel(t1, tm), rel(t0, t1), rel(lo[:, 2], lo[:, 1]), rel(hi[:, 0], hi[:, 1])])


class PathSpec:
    def __init__(self, sd, sample_root, max_trace_depth, seed):
        self.sd = sd
        self.n, self.N, self.D, self.seed = sample_root, sample_root * sample_root, max_trace_depth, seed
        self.width, self.height = sd.output_settings.image_width, sd.output_settings.image_height
        # the restatement's context: spheres, planes and meshes only, in their order; _analytic[k] / _mesh_of_tri[k] give the YAML index
        known, self._analytic, self._mesh_of_tri = [], [], []
        for i, s in enumerate(sd.shapes):
            if _kind(s) in ("SphereData", "PlaneData", "MeshData"):
                s = copy.copy(s)
                if _kind(s.material) == "DielectricData":
                    s.material = _STAND_IN
                known.append(s)
                if _kind(s) == "MeshData":
                    self._mesh_of_tri += [i] * len(np.asarray(s.triangles).reshape(-1, 3))
                else:
                    self._analytic.append(i)
        osd = copy.copy(sd)
        osd.shapes = known
        cfg = types.SimpleNamespace(sample_root=sample_root, max_trace_depth=max_trace_depth, rows_per_work_unit=50)
        self._oracle = oracle_mod.Oracle(osd, cfg, seed=seed)
        self._hemi = self._oracle.hemi_sets()    # [S][D][N][3]
        self._pixel = self._oracle.pixel_sets()  # [S][N][2]
        self._has_extension = any(_kind(s) in ("DiskData", "BoxData") for s in sd.shapes)
        self._params = {i: oracle_mod.material_params(s.material) for i, s in enumerate(sd.shapes)
                        if _kind(s.material) != "DielectricData"}
        self.background = np.asarray(sd.background, dtype=np.float64)
        self.stats = None
        self.margins = {k: np.inf for k in MARGIN_NAMES}
        self.classes = collections.Counter()
        self._frame = None

    def close(self):
        self._oracle.close()

    # ---- the nearest hit ------------------------------------------------------------------------------------------------------

    def _note(self, margins, name, values):
        v = np.asarray(values, dtype=np.float64).ravel()
        v = v[np.isfinite(v)]
        if v.size:
            margins[name] = min(margins[name], float(v.min()))

    def _known_margins(self, o, d, margins):
        """Candidate t of every sphere and plane, [m] each, in numpy -- for the margins only."""
        cands = []
        for i in self._analytic:
            s = self.sd.shapes[i]
            if _kind(s) == "SphereData":
                temp = o - np.asarray(s.center, dtype=np.float64)
                a, b, c = _dot(d, d), 2.0 * _dot(temp, d), _dot(temp, temp) - s.radius * s.radius
                disc = b * b - 4.0 * a * c
                self._note(margins, "sphere_discriminant", np.abs(disc) / (b * b))
                e = np.sqrt(np.where(disc >= 0.0, disc, np.nan))
                t1, t2 = (-b - e) / (2.0 * a), (-b + e) / (2.0 * a)
                self._note(margins, "t_min", [np.abs(t1 - T_MIN) / T_MIN, np.abs(t2 - T_MIN) / T_MIN])
                t = np.where(t1 > T_MIN, t1, np.where(t2 > T_MIN, t2, np.inf))
            else:
                n = np.asarray(s.normal, dtype=np.float64)
                t = _dot(np.asarray(s.point, dtype=np.float64) - o, n[None, :]) / _dot(d, n[None, :])
                self._note(margins, "t_min", np.abs(t - T_MIN) / T_MIN)
                t = np.where(t > T_MIN, t, np.inf)
            cands.append(np.where(np.isnan(t), np.inf, t))
        return cands

    def _nearest(self, o, d, margins):
        """Rays o, d [m, 3]: (YAML index [m], -1 on a miss; t; normal [m, 3]; hit point [m, 3]; box face [m], -1 elsewhere;
        on a triangle [m])."""
        m = len(o)
        shape, face = np.full(m, -1), np.full(m, -1)
        t, nrm, pt = np.full(m, np.inf), np.zeros((m, 3)), np.zeros((m, 3))
        found, tri = np.zeros(m, bool), np.zeros(m, bool)
        for j in range(m):
            idx, tt, nn, pp = self._oracle.scene_hit(o[j], d[j])
            if idx >= 0:
                k = idx - len(self._analytic)
                found[j], tri[j] = True, k >= 0
                shape[j] = self._mesh_of_tri[k] if k >= 0 else self._analytic[idx]
                t[j], nrm[j], pt[j] = tt, nn, pp
        cands = self._known_margins(o, d, margins)
        cands.append(np.where(tri, t, np.inf))
        for i, s in enumerate(self.sd.shapes):
            if _kind(s) == "DiskData":
                hit, te, dist2 = disk_hit(s.center, s.normal, s.radius, o, d)
                r2 = s.radius * s.radius
                reach = np.isfinite(te) & (te > T_MIN)
                self._note(margins, "disk_rim", np.where(reach, np.abs(dist2 - r2), np.nan) / r2)
                self._note(margins, "t_min", np.abs(te - T_MIN) / T_MIN)
                ne, fe = np.broadcast_to(np.asarray(s.normal, dtype=np.float64), (m, 3)), np.full(m, -1)
            elif _kind(s) == "BoxData":
                hit, te, ne, fe, parts = box_spec.box_hit(s.corner0, s.corner1, o, d, invert=s.invert)
                self._note(margins, "box_rounding_level", box_margin(*parts))
            else:
                continue
            cands.append(np.where(hit, te, np.inf))
            take = hit & (~found | (te < t) | ((te == t) & (tri | (i < shape))))
            pe = o + te[:, None] * d
            shape, face, t = np.where(take, i, shape), np.where(take, fe, face), np.where(take, te, t)
            nrm, pt = np.where(take[:, None], ne, nrm), np.where(take[:, None], pe, pt)
            tri, found = tri & ~take, found | take
        if len(cands) >= 2:
            two = np.sort(np.stack(cands, axis=1), axis=1)[:, :2]
            self._note(margins, "nearest_gap", (two[:, 1] - two[:, 0]) / np.abs(two[:, 0]))
        return shape, t, nrm, pt, face, tri

    # ---- Scene::shade ---------------------------------------------------------------------------------------------------------

    def _materials(self, shape, o, d, tri, depth):
        """Where the material of a hit is chosen, for this class and for the loops of aov_chain_spec: for the rays o, d [m, 3] of
        segment `depth` with nearest hits `shape` [m] (`tri` [m]: on a triangle), per ray (the shape's material, its cached
        material_params -- None for a Dielectric, which has none), or None for a miss.  A subclass may put another material on a hit."""
        return [None if si < 0 else (self.sd.shapes[si].material, self._params.get(int(si))) for si in shape]

    def _trace(self, o, d, sets, idx):
        """The paths of primary rays o, d [k, 3] of sample sets `sets` and sample indices `idx`: (radiance [k, 3], statistics,
        margins, classes, first hits: shape, t, normal and _materials' choice)."""
        with np.errstate(all="ignore"):
            return self._trace_quiet(np.array(o, dtype=np.float64), np.array(d, dtype=np.float64), sets, idx)

    def _trace_quiet(self, o, d, sets, idx):
        k = len(o)
        st = dict.fromkeys(STAT_NAMES, 0)
        st["samples"] = k
        margins, classes = {name: np.inf for name in MARGIN_NAMES}, collections.Counter()
        end = np.zeros((k, 3))  # the radiance at each path's end: an emitter's, the background, or 0 at the depth limit
        bounces = []            # per depth: (rays, f [m, 3], n.wi / pdf [m])
        live = np.arange(k)
        first = None
        for depth in range(1, self.D + 2):
            if depth > self.D:
                st["depth_exhausted"] += len(live)
                break
            if not len(live):
                break
            st["segments"] += len(live)
            shape, t, nrm, pt, face, tri = self._nearest(o[live], d[live], margins)
            chosen = self._materials(shape, o[live], d[live], tri, depth)
            if depth == 1:
                first = (shape.copy(), t.copy(), nrm.copy(), chosen)
            rays, fs, scales = [], [], []
            for j, ray in enumerate(live):
                si = int(shape[j])
                if si < 0:
                    st["misses"] += 1
                    end[ray] = self.background
                    continue
                s, n, dr = self.sd.shapes[si], nrm[j], d[ray]
                mat = chosen[j][0]
                classes[_kind(s)[:-4] + "/" + _kind(mat)[:-4]] += 1
                if face[j] >= 0:
                    classes[f"box face {int(face[j])}"] += 1
                    classes["inverted box"] += bool(s.invert)
                if tri[j] and self._has_extension:
                    classes["triangle beside a disk or box"] += 1
                if _kind(mat) == "EmissiveData":  # materials.rs:41-50
                    st["emissive_hits"] += 1
                    facing = _dot(n * -1.0, dr)
                    self._note(margins, "emitter_facing", abs(facing) / np.sqrt(_dot(n, n) * _dot(dr, dr)))
                    if facing > 0.0:
                        end[ray] = np.asarray(mat.color, dtype=np.float64) * mat.power
                    continue
                if _kind(mat) == "DielectricData":
                    u = self._hemi[sets[ray], depth - 1, idx[ray], 2]
                    refl, wi, F = dielectric_spec.bounce(n[None, :], dr[None, :], mat.refraction_index, np.array([u]))
                    self._note(margins, "fresnel", abs(u - F[0]))
                    if refl[0]:
                        st["dielectric_reflections"] += 1
                        classes["total internal reflection" if F[0] == 1.0 else "reflection"] += 1
                        f = np.ones(3)
                    else:
                        st["dielectric_transmissions"] += 1
                        classes["transmission"] += 1
                        f = np.asarray(mat.transmit_color, dtype=np.float64)
                    wi, scale = wi[0], 1.0
                else:  # materials.rs:18-34, 56-72
                    mk, mp = chosen[j][1]
                    st[{oracle_mod.MAT_MATTE: "matte_bounces", oracle_mod.MAT_GLOSSY: "glossy_bounces",
                        oracle_mod.MAT_REFLECTIVE: "specular_bounces"}[mk]] += 1
                    sq = self._pixel[sets[ray], idx[ray]]
                    wi, pdf, f = oracle_mod.sample_f(mk, mp, n, dr * -1.0, self._hemi[sets[ray], depth - 1, idx[ray]], sq)
                    scale = _dot(n, wi) / np.float64(pdf)
                    if mk == oracle_mod.MAT_GLOSSY:
                        self._note(margins, "glossy_flip", self._glossy_flip_margin(n, dr, sq, mat.reflect_exponent))
                rays.append(ray)
                fs.append(f)
                scales.append(scale)
                o[ray], d[ray] = pt[j], wi
            live = np.array(rays, dtype=int)
            bounces.append((live, np.array(fs).reshape(-1, 3), np.array(scales)))
        rad = end
        for rays, f, scale in reversed(bounces):  # rgb_scale(rgb_mul(f, child), n.wi / pdf), the deepest bounce first
            if len(rays):
                rad[rays] = (f * rad[rays]) * scale[:, None]
        return rad, st, margins, classes, first

    @staticmethod
    def _glossy_flip_margin(n, dr, sq, exponent):
        """|n.wi0| / (|n| |wi0|) of GlossySpecular::sample_f's unmirrored direction (brdf.rs:57-66), in numpy, for the margin only."""
        wo = dr * -1.0
        w = -wo + n * _dot(n, wo) * 2.0
        u = np.cross(np.array([0.00424, 1.0, 0.00764]), w)
        u = u / np.sqrt(_dot(u, u))
        v = np.cross(u, w)
        hs = oracle_mod.to_unit_hemi(sq[0], sq[1], exponent)
        wi0 = (u * hs[0] + v * hs[1]) + w * hs[2]
        return abs(_dot(n, wi0)) / np.sqrt(_dot(n, n) * _dot(wi0, wi0))

    # ---- the frame ------------------------------------------------------------------------------------------------------------

    def primary_rays(self):
        """(o, d, set) of every sample: [H, W, N, 3] twice and [H, W]."""
        H, W, N = self.height, self.width, self.N
        o, d, sets = np.empty((H, W, N, 3)), np.empty((H, W, N, 3)), np.empty((H, W), dtype=int)
        for row in range(H):
            perm = self._oracle.row_perm(row)
            for col in range(W):
                sets[row, col] = int(perm[col]) % W
                for i in range(N):
                    o[row, col, i], d[row, col, i] = self._oracle.primary_ray(row, col, sets[row, col], i)
        return o, d, sets

    def frame(self):
        """[H, W, 3]: per pixel the mean over its samples in index order, then max_to_one, as render_row (trace.rs:63-91) has it."""
        if self._frame is not None:
            return self._frame
        H, W, N = self.height, self.width, self.N
        o, d, sets = self.primary_rays()
        rad, self.stats, self.margins, self.classes, first = self._trace(
            o.reshape(-1, 3), d.reshape(-1, 3), np.repeat(sets.ravel(), N), np.tile(np.arange(N), H * W))
        self.sample_radiance = rad.reshape(H, W, N, 3)
        self.primary = (o, d, sets)
        self._first = (first[0].reshape(H, W, N), first[1].reshape(H, W, N), first[2].reshape(H, W, N, 3))
        self._first_materials = first[3]
        with np.errstate(all="ignore"):
            color = np.zeros((H, W, 3))
            for i in range(N):
                color = color + self.sample_radiance[:, :, i]
            color = color * (1.0 / float(N))
        self._frame = np.array([[oracle_mod.max_to_one(color[r, c]) for c in range(W)] for r in range(H)])
        return self._frame

    def sample(self, row, col, index):
        """The radiance of one sample, traced on its own."""
        s = int(self._oracle.row_perm(row)[col]) % self.width
        o, d = self._oracle.primary_ray(row, col, s, index)
        return self._trace(o[None, :], d[None, :], np.array([s]), np.array([index]))[0][0]

    def first_hits(self):
        """Per sample [H, W, N]: the YAML index of the depth-1 hit (-1 for a miss), its t and its normal [H, W, N, 3]."""
        self.frame()
        return self._first

    def first_materials(self):
        """Per sample, flat in [H, W, N] order: what _materials chose for the depth-1 hit, None for a miss."""
        self.frame()
        return self._first_materials

    def min_margin(self):
        self.frame()
        return min(self.margins.values())


def aov_buffers(spec):
    """The first-hit feature buffers of a PathSpec, built with aov_spec's albedo and _finish."""
    import aov_spec
    shape, t, nrm = spec.first_hits()
    chosen = spec.first_materials()
    _, d, _ = spec.primary
    H, W, N = shape.shape
    alb, nsum, tsum, hits = np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros((H, W)), np.zeros((H, W))
    for r in range(H):
        for c in range(W):
            for i in range(N):
                si = int(shape[r, c, i])
                if si < 0:
                    alb[r, c] += spec.background
                    continue
                alb[r, c] += aov_spec.albedo(chosen[(r * W + c) * N + i][0], nrm[r, c, i], d[r, c, i])
                nsum[r, c] += nrm[r, c, i]
                tsum[r, c] += t[r, c, i]
                hits[r, c] += 1
    return aov_spec._finish(alb, nsum, tsum, hits, N)
