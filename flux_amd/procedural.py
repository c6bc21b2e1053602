"""Procedural triangle scenes (extension: the reference has no triangles, so it defines no such scene;
BASELINE.json config 5 asks for a "procedural 1M-triangle scene (stress BVH)").

heightfield_scene() is fully specified here so that the CPU checker, the GPU path and any future reader
build the identical mesh:

  * demo2.yml's camera, output settings, background, environment sphere (shape 0) and area light
    (shape 1) and its ten glossy spheres (shapes 2..11) are kept; demo2's ground Plane is replaced by
  * an infinite Matte plane at y = -1 (catches rays that leave the height field), and
  * ONE Matte (0.5,0.5,0.5; kd 1) mesh: a regular (nx+1) x (nz+1) vertex grid over
    x in [-14, 14], z in [-10, 20]; vertex (i,j) at x = -14 + 28 i/nx, z = -10 + 30 j/nz,
    y = 0.35 sin(1.7 x) cos(1.3 z) + 0.02 (2 u_ij - 1), u_ij = numpy default_rng(seed).random((nx+1, nz+1))[i, j];
    cell (i,j) gives triangles (v00, v01, v11) and (v00, v11, v10) with v_ab = vertex (i+a, j+b),
    cells in i-major order -> 2 nx nz triangles (nx=1000, nz=500: exactly 1,000,000).
"""
import copy
import os

import numpy as np

from .scene import MatteData, MeshData, PlaneData, SceneData, load_scene

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def vertex_normals(vertices, triangles) -> np.ndarray:
    """Area-weighted vertex normals, float64 [nv][3]: per vertex the sum of (v1 - v0) x (v2 - v0) -- twice the area times the facet
    normal -- over the triangles that use it, in triangle order, normalised.  A vertex no triangle with an area uses gets (0, 1, 0),
    so that the result is always a valid MeshData.normals."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    face = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    n = np.zeros_like(v)
    for c in range(3):
        np.add.at(n, t[:, c], face)
    length = np.sqrt((n * n).sum(axis=1))
    ok = np.isfinite(length) & (length > 0.0)
    n[~ok] = (0.0, 1.0, 0.0)
    length[~ok] = 1.0
    return n / length[:, None]


def elevation_colors(vertices, low_rgb, high_rgb) -> np.ndarray:
    """Per-vertex colours, float64 [nv][3]: a linear ramp from `low_rgb` at the mesh's lowest y to `high_rgb` at its highest
    (low + s (high - low), s = (y - y_min) / (y_max - y_min); a mesh of one height gets `low_rgb`)."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    lo, hi = np.asarray(low_rgb, dtype=np.float64), np.asarray(high_rgb, dtype=np.float64)
    y0, y1 = (float(v[:, 1].min()), float(v[:, 1].max())) if len(v) else (0.0, 0.0)
    s = (v[:, 1] - y0) / (y1 - y0) if y1 > y0 else np.zeros(len(v))
    return lo + np.clip(s, 0.0, 1.0)[:, None] * (hi - lo)


def uv_sphere_mesh(segments: int, rings: int, center=(0.0, 0.0, 0.0), radius: float = 1.0, material=None, smooth: bool = True,
                   colors=None) -> MeshData:
    """A latitude / longitude sphere: `segments` around the y axis, `rings` from pole to pole, 2 segments (rings - 1) triangles --
    a fan of `segments` triangles at each pole and a quad (two triangles sharing their first vertex and an edge, facing outwards)
    per segment and inner ring.  Vertices: the north pole, (rings - 1) rows of `segments`, the south pole.  smooth: the exact
    sphere normals (vertex - center) / radius as per-vertex `normals`.  colors: MeshData.colors, per vertex or per corner."""
    if segments < 3 or rings < 2:
        raise ValueError("uv_sphere_mesh: segments >= 3 and rings >= 2 required")
    c = np.asarray(center, dtype=np.float64)
    theta = np.pi * np.arange(1, rings, dtype=np.float64) / rings
    phi = 2.0 * np.pi * np.arange(segments, dtype=np.float64) / segments
    T, P = np.meshgrid(theta, phi, indexing="ij")
    unit = np.concatenate([[[0.0, 1.0, 0.0]],
                           np.stack([np.sin(T) * np.cos(P), np.cos(T), np.sin(T) * np.sin(P)], axis=-1).reshape(-1, 3),
                           [[0.0, -1.0, 0.0]]])
    south = len(unit) - 1

    def vid(r, s):
        return 1 + r * segments + s % segments
    tris = []
    for s in range(segments):
        tris.append((0, vid(0, s + 1), vid(0, s)))
    for r in range(rings - 2):
        for s in range(segments):
            a, b, d, e = vid(r, s), vid(r, s + 1), vid(r + 1, s + 1), vid(r + 1, s)
            tris.append((a, b, d))
            tris.append((a, d, e))
    for s in range(segments):
        tris.append((south, vid(rings - 2, s), vid(rings - 2, s + 1)))
    if material is None:
        material = MatteData((0.5, 0.5, 0.5), (1.0, 1.0, 1.0), 1.0)
    return MeshData(c + radius * unit, np.array(tris, dtype=np.uint32), material, unit.copy() if smooth else None, colors)


# heightfield_mesh(colored=True): valley to crest
ELEVATION_LOW, ELEVATION_HIGH = (0.25, 0.55, 0.2), (1.0, 0.95, 0.9)


def heightfield_mesh(nx: int, nz: int, seed: int = 12345, smooth: bool = False, colored: bool = False) -> MeshData:
    i = np.arange(nx + 1, dtype=np.float64)
    j = np.arange(nz + 1, dtype=np.float64)
    x = -14.0 + 28.0 * i / nx
    z = -10.0 + 30.0 * j / nz
    X, Z = np.meshgrid(x, z, indexing="ij")
    u = np.random.default_rng(seed).random((nx + 1, nz + 1))
    Y = 0.35 * np.sin(1.7 * X) * np.cos(1.3 * Z) + 0.02 * (2.0 * u - 1.0)
    verts = np.stack([X, Y, Z], axis=-1).reshape(-1, 3)

    def vid(a, b):
        return (a * (nz + 1) + b).astype(np.uint32)

    I, J = np.meshgrid(np.arange(nx), np.arange(nz), indexing="ij")
    I, J = I.reshape(-1), J.reshape(-1)
    v00, v01, v11, v10 = vid(I, J), vid(I, J + 1), vid(I + 1, J + 1), vid(I + 1, J)
    tris = np.empty((nx * nz, 2, 3), dtype=np.uint32)
    tris[:, 0, 0], tris[:, 0, 1], tris[:, 0, 2] = v00, v01, v11
    tris[:, 1, 0], tris[:, 1, 1], tris[:, 1, 2] = v00, v11, v10
    tris = tris.reshape(-1, 3)
    return MeshData(verts, tris, MatteData((0.5, 0.5, 0.5), (1.0, 1.0, 1.0), 1.0), vertex_normals(verts, tris) if smooth else None,
                    elevation_colors(verts, ELEVATION_LOW, ELEVATION_HIGH) if colored else None)


def heightfield_scene(nx: int = 1000, nz: int = 500, seed: int = 12345, base: SceneData = None, smooth: bool = False,
                      colored: bool = False) -> SceneData:
    sd = copy.deepcopy(base) if base is not None else load_scene(os.path.join(_ROOT, "scenes", "demo2.yml"))
    sd.scene_name = f"heightfield_{nx}x{nz}"
    shapes = [s for s in sd.shapes if not isinstance(s, PlaneData)]
    shapes.append(PlaneData((0.0, -1.0, 0.0), (0.0, 1.0, 0.0), MatteData((0.5, 0.5, 0.5), (1.0, 1.0, 1.0), 1.0)))
    shapes.append(heightfield_mesh(nx, nz, seed, smooth, colored))
    sd.shapes = shapes
    return sd
