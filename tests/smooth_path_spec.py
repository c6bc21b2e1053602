"""The full-path reference (tests/path_spec.py) for scenes whose meshes carry corner normals: PathSpec with the
normal of a triangle hit replaced by smooth_spec's.  The triangle is identified from the restatement's hit index (triangles follow
the analytic shapes there, meshes in their order), its record (v0, e1, e2) is the host build's, and the fall-back is the normal the
restatement itself reports -- so a scene without normals goes through PathSpec's own values untouched.

One margin more than PathSpec's: "smooth_l2", |l2 - 1e-24| / max(l2, 1e-24) of every interpolated normal."""
import numpy as np

import smooth_spec
from flux_amd.scene import corner_normals
from path_spec import PathSpec, _kind

MARGIN_NAMES_SMOOTH = ("smooth_l2",)


class SmoothPathSpec(PathSpec):
    def __init__(self, sd, sample_root, max_trace_depth, seed):
        super().__init__(sd, sample_root, max_trace_depth, seed)
        v0, e1, e2, on, cn = [], [], [], [], []
        for s in sd.shapes:
            if _kind(s) != "MeshData":
                continue
            a, b, c, _ = smooth_spec.mesh_triangles(s)
            corners = corner_normals(s)
            v0.append(a), e1.append(b), e2.append(c)
            on.append(np.full(len(a), corners is not None))
            cn.append(np.zeros((len(a), 3, 3)) if corners is None else smooth_spec.normalize(corners))
        cat = lambda xs, shape: np.concatenate(xs) if xs else np.zeros(shape)  # noqa: E731
        self._v0, self._e1, self._e2 = cat(v0, (0, 3)), cat(e1, (0, 3)), cat(e2, (0, 3))
        self._smooth, self._corners = cat(on, (0,)).astype(bool), cat(cn, (0, 3, 3))
        self.margins.update({k: np.inf for k in MARGIN_NAMES_SMOOTH})

    def triangle_of(self, o, d):
        """The index (meshes concatenated in their order) of the triangle the restatement reports for the ray, or -1"""
        idx = self._oracle.scene_hit(o, d)[0]
        return idx - len(self._analytic) if idx >= len(self._analytic) else -1

    def _nearest(self, o, d, margins):
        shape, t, nrm, pt, face, tri = super()._nearest(o, d, margins)
        margins.setdefault("smooth_l2", np.inf)
        if self._smooth.any():
            nrm = np.array(nrm)
            for j in np.flatnonzero(tri):
                k = self.triangle_of(o[j], d[j])
                if k < 0 or not self._smooth[k]:
                    continue
                u, v = smooth_spec.barycentrics(self._v0[k], self._e1[k], self._e2[k], o[j], d[j])
                c = self._corners[k]
                nrm[j], l2 = smooth_spec.interpolate(u, v, c[0], c[1], c[2], nrm[j])
                self._note(margins, "smooth_l2", abs(l2 - smooth_spec.L2_MIN) / max(l2, smooth_spec.L2_MIN))
        return shape, t, nrm, pt, face, tri
