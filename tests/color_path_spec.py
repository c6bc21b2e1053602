"""The full-path reference (tests/path_spec.py, tests/smooth_path_spec.py) for scenes whose meshes carry corner colours (DESIGN.md
§5k): SmoothPathSpec with the colour of the material of a triangle hit replaced by colour (*) c, c being color_spec's factor at the
hit.  The triangle is identified as SmoothPathSpec.triangle_of does it, its record (v0, e1, e2) is the host build's, and the stored
colours are color_spec.store's f32.

PathSpec._trace_quiet has no seam where the material's colour enters, so the loop is restated here with one change: the material
goes through `_tinted` before material_params / sample_f / the Emissive end.  tests/test_color_path_spec.py pins the restated loop
to SmoothPathSpec bit for bit on scenes without colours and with all-ones colours.  The feature buffers get twins likewise:
aov_buffers (path_spec.aov_buffers) and chain_buffers (aov_chain_spec.chain_buffers) with the tinted albedo."""
import collections
import dataclasses

import numpy as np

import aov_chain_spec
import aov_spec
import color_spec
import dielectric_spec
import smooth_spec
from flux_amd.scene import corner_colors
from oracle import oracle as oracle_mod
from path_spec import MARGIN_NAMES, STAT_NAMES, _dot, _kind
from smooth_path_spec import SmoothPathSpec

COLOR_FIELD = {"MatteData": "diffuse_color", "ReflectiveData": "reflect_color", "GlossyReflectiveData": "reflect_color",
               "DielectricData": "transmit_color", "EmissiveData": "color"}


def _tinted(mat, c):
    """`mat` with its colour multiplied by the factor c [3], per channel; c None: `mat` itself"""
    if c is None:
        return mat
    field = COLOR_FIELD[_kind(mat)]
    return dataclasses.replace(mat, **{field: tuple(float(x) for x in np.asarray(getattr(mat, field), dtype=np.float64) * c)})


class ColorPathSpec(SmoothPathSpec):
    def __init__(self, sd, sample_root, max_trace_depth, seed):
        super().__init__(sd, sample_root, max_trace_depth, seed)
        on, st = [], []
        for s in sd.shapes:
            if _kind(s) != "MeshData":
                continue
            nt = len(np.asarray(s.triangles).reshape(-1, 3))
            corners = corner_colors(s)
            on.append(np.full(nt, corners is not None))
            st.append(np.zeros((nt, 3, 3), dtype=np.float32) if corners is None else color_spec.store(corners))
        self._colored = np.concatenate(on).astype(bool) if on else np.zeros(0, bool)
        self._stored = np.concatenate(st) if st else np.zeros((0, 3, 3), dtype=np.float32)
        if not self._smooth.any():   # (SmoothPathSpec keeps the records only as far as it needs them)
            tri = [smooth_spec.mesh_triangles(s)[:3] for s in sd.shapes if _kind(s) == "MeshData"]
            if tri:
                self._v0, self._e1, self._e2 = (np.concatenate(x) for x in zip(*tri))
        self._first_factor = None

    def factors(self, o, d, tri):
        """Per ray of o, d [m, 3]: the colour factor [3] of the triangle hit, or None where the hit is not on a coloured triangle"""
        out = [None] * len(o)
        if self._colored.any():
            for j in np.flatnonzero(tri):
                k = self.triangle_of(o[j], d[j])
                if k >= 0 and self._colored[k]:
                    out[j] = color_spec.color_factor(self._v0[k], self._e1[k], self._e2[k], self._stored[k], o[j], d[j])
        return out

    def _trace_quiet(self, o, d, sets, idx):
        k = len(o)
        st = dict.fromkeys(STAT_NAMES, 0)
        st["samples"] = k
        margins, classes = {name: np.inf for name in MARGIN_NAMES}, collections.Counter()
        end = np.zeros((k, 3))
        bounces = []
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
            factor = self.factors(o[live], d[live], tri)
            if depth == 1:
                first = (shape.copy(), t.copy(), nrm.copy())
                self._last_first_factor = factor
            rays, fs, scales = [], [], []
            for j, ray in enumerate(live):
                si = int(shape[j])
                if si < 0:
                    st["misses"] += 1
                    end[ray] = self.background
                    continue
                s, n, dr = self.sd.shapes[si], nrm[j], d[ray]
                mat = _tinted(s.material, factor[j])   # <- the one change against PathSpec._trace_quiet
                classes[_kind(s)[:-4] + "/" + _kind(mat)[:-4]] += 1
                if face[j] >= 0:
                    classes[f"box face {int(face[j])}"] += 1
                    classes["inverted box"] += bool(s.invert)
                if tri[j] and self._has_extension:
                    classes["triangle beside a disk or box"] += 1
                if _kind(mat) == "EmissiveData":
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
                else:
                    mk, mp = self._params[si] if factor[j] is None else oracle_mod.material_params(mat)
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
        for rays, f, scale in reversed(bounces):
            if len(rays):
                rad[rays] = (f * rad[rays]) * scale[:, None]
        return rad, st, margins, classes, first

    def frame(self):
        if self._frame is None:
            super().frame()
            self._first_factor = self._last_first_factor   # per sample, flat in [H, W, N] order
        return self._frame

    def first_factors(self):
        self.frame()
        return self._first_factor


def aov_buffers(spec):
    """path_spec.aov_buffers of a ColorPathSpec, with the tinted material's albedo"""
    shape, t, nrm = spec.first_hits()
    factor = spec.first_factors()
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
                mat = _tinted(spec.sd.shapes[si].material, factor[(r * W + c) * N + i])
                alb[r, c] += aov_spec.albedo(mat, nrm[r, c, i], d[r, c, i])
                nsum[r, c] += nrm[r, c, i]
                tsum[r, c] += t[r, c, i]
                hits[r, c] += 1
    return aov_spec._finish(alb, nsum, tsum, hits, N)


def chain_buffers(spec, max_chain=0):
    """aov_chain_spec.chain_buffers of a ColorPathSpec: its loop restated with the material of a hit tinted.  Returns (buffers
    [H, W, 8], margins)."""
    with np.errstate(all="ignore"):
        return _chain_quiet(spec, aov_chain_spec.limit(spec, max_chain))


def _chain_quiet(spec, K):
    o0, d0, sets = aov_chain_spec._primary(spec)
    Hh, Ww, N = o0.shape[:3]
    o, d = o0.reshape(-1, 3).copy(), d0.reshape(-1, 3).copy()
    m = len(o)
    set_of, idx_of = np.repeat(sets.ravel(), N), np.tile(np.arange(N), Hh * Ww)
    margins = {name: np.inf for name in MARGIN_NAMES}
    end, nrm, depth, covered, tsum = np.zeros((m, 3)), np.zeros((m, 3)), np.zeros(m), np.zeros(m, bool), np.zeros(m)
    bounces = []
    live = np.arange(m)
    for k in range(1, K + 1):
        if not len(live):
            break
        shape, t, n_hit, pt, _, tri = spec._nearest(o[live], d[live], margins)
        factor = spec.factors(o[live], d[live], tri)
        rays, fs, scales = [], [], []
        for j, ray in enumerate(live):
            si = int(shape[j])
            if si < 0:
                end[ray] = spec.background
                continue
            mat, n, dr = _tinted(spec.sd.shapes[si].material, factor[j]), n_hit[j], d[ray]
            if _kind(mat) in aov_chain_spec.DELTA and k < K:
                if _kind(mat) == "DielectricData":
                    u = spec._hemi[set_of[ray], k - 1, idx_of[ray], 2]
                    refl, wi, F = dielectric_spec.bounce(n[None, :], dr[None, :], mat.refraction_index, np.array([u]))
                    spec._note(margins, "fresnel", abs(u - F[0]))
                    f = np.ones(3) if refl[0] else np.asarray(mat.transmit_color, dtype=np.float64)
                    wi, scale = wi[0], 1.0
                else:
                    mk, mp = oracle_mod.material_params(mat)
                    wi, pdf, f = oracle_mod.sample_f(mk, mp, n, dr * -1.0, spec._hemi[set_of[ray], k - 1, idx_of[ray]],
                                                     spec._pixel[set_of[ray], idx_of[ray]])
                    scale = _dot(n, wi) / np.float64(pdf)
                rays.append(ray)
                fs.append(f)
                scales.append(scale)
                tsum[ray] += t[j]
                o[ray], d[ray] = pt[j], wi
                continue
            if _kind(mat) == "EmissiveData":
                spec._note(margins, "emitter_facing", abs(_dot(n * -1.0, dr)) / np.sqrt(_dot(n, n) * _dot(dr, dr)))
            end[ray] = aov_spec.albedo(mat, n, dr)
            nrm[ray], depth[ray], covered[ray] = n, tsum[ray] + t[j], True
        live = np.array(rays, dtype=int)
        bounces.append((live, np.array(fs).reshape(-1, 3), np.array(scales)))
    alb = end
    for rays, f, scale in reversed(bounces):
        if len(rays):
            alb[rays] = (f * alb[rays]) * scale[:, None]
    alb, nrm = alb.reshape(Hh, Ww, N, 3), nrm.reshape(Hh, Ww, N, 3)
    depth, covered = depth.reshape(Hh, Ww, N), covered.reshape(Hh, Ww, N)
    asum, nsum, tsums, hits = np.zeros((Hh, Ww, 3)), np.zeros((Hh, Ww, 3)), np.zeros((Hh, Ww)), np.zeros((Hh, Ww))
    for i in range(N):
        asum = asum + alb[:, :, i]
        c = covered[:, :, i]
        nsum = nsum + np.where(c[..., None], nrm[:, :, i], 0.0)
        tsums = tsums + np.where(c, depth[:, :, i], 0.0)
        hits = hits + c
    return aov_spec._finish(asum, nsum, tsums, hits, N), margins
