"""The full-path reference (tests/path_spec.py, tests/smooth_path_spec.py) for scenes whose meshes carry corner colours (DESIGN.md
§5k): SmoothPathSpec with the colour of the material of a triangle hit replaced by colour (*) c, c being color_spec's factor at the
hit.  The triangle is identified as SmoothPathSpec.triangle_of does it, its record (v0, e1, e2) is the host build's, and the stored
colours are color_spec.store's f32.

The colour enters at PathSpec._materials, the one point where the path loop, path_spec.aov_buffers and aov_chain_spec's chain loop
ask for the material of a hit: the override sends it through `_tinted` before material_params / sample_f / the Emissive end / the
albedo.  tests/test_color_path_spec.py pins the override to SmoothPathSpec bit for bit on scenes without colours and with all-ones
colours."""
import dataclasses

import numpy as np

import aov_chain_spec
import color_spec
import path_spec
import smooth_spec
from flux_amd.scene import corner_colors
from oracle import oracle as oracle_mod
from path_spec import _kind
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

    def _materials(self, shape, o, d, tri, depth):
        """PathSpec's choice with the material of a hit on a coloured triangle tinted; every other hit keeps PathSpec's own pair"""
        factor = self.factors(o, d, tri)
        if depth == 1:
            self._last_first_factor = factor
        out = super()._materials(shape, o, d, tri, depth)
        for j, c in enumerate(factor):
            if c is not None:
                mat = _tinted(out[j][0], c)
                out[j] = (mat, None if _kind(mat) == "DielectricData" else oracle_mod.material_params(mat))
        return out

    def frame(self):
        if self._frame is None:
            super().frame()
            self._first_factor = self._last_first_factor   # per sample, flat in [H, W, N] order
        return self._frame

    def first_factors(self):
        self.frame()
        return self._first_factor


def aov_buffers(spec):
    """path_spec.aov_buffers: the albedo is the tinted material's, through ColorPathSpec._materials"""
    return path_spec.aov_buffers(spec)


def chain_buffers(spec, max_chain=0):
    """aov_chain_spec.chain_buffers, likewise, as (buffers [H, W, 8], margins)"""
    chain = aov_chain_spec.chain_buffers(spec, max_chain)
    return chain.buffers, chain.margins
