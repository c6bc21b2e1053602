"""Renderer: the Scene + Camera pair of the reference, backed by the HIP library.

    Scene::from_data(job.scene_data, job.config)     fluxcore/src/workers.rs:46
    Camera::new(..., num_sets = image_width, ...)    fluxcore/src/workers.rs:47-54
    camera.render(&scene, unit) -> WorkUnitResult    fluxcore/src/workers.rs:60

All compute happens in libflux_hip.so on the GPU; there is no CPU path here.
"""
import ctypes as C

import numpy as np

from . import _lib
from .scene import JobConfiguration, SceneData, SceneDesc, WorkUnit, WorkUnitResult, MESH_ATTRIBUTES, _corner_attribute, split_shapes

STAT_NAMES = ("samples", "segments", "matte_bounces", "glossy_bounces", "specular_bounces",
              "emissive_hits", "misses", "depth_exhausted", "bvh_nodes", "tris_tested",
              "dielectric_reflections", "dielectric_transmissions")


class Renderer:
    def __init__(self, scene_data: SceneData, config: JobConfiguration, seed: int = 1, device: int = 0,
                 set_share=None):
        """`set_share` = (first_set, set_stride): hold the sample tables of this rank's sets only
        (flux_ctx_create_sets; render with render_sets_device)."""
        self.scene_data = scene_data
        self.config = config
        self.seed = int(seed)
        self.device = int(device)
        self.width = scene_data.output_settings.image_width
        self.height = scene_data.output_settings.image_height
        self._desc = SceneDesc(scene_data)
        cfg = _lib.FluxJobCfg(config.sample_root, config.max_trace_depth, config.rows_per_work_unit)
        h = C.c_void_p()
        self.set_share = (0, 1) if set_share is None else (int(set_share[0]), int(set_share[1]))
        _lib.check(_lib.lib.flux_ctx_create_sets(C.byref(self._desc.desc), C.byref(cfg), C.c_uint64(self.seed),
                                                 self.device, self.set_share[0], self.set_share[1], C.byref(h)))
        self._h = h
        _set_scene_attributes(h, scene_data)
        self._warn_if_routed()

    def _warn_if_routed(self):
        """FLUX_MATH_FAST is defined for unit surface normals; a scene with a NON-unit plane normal is rendered with the STRICT
        arithmetic (about 3.5 x slower, no traversal kernels for meshes) whatever set_math says -- reported once per renderer
        instead of being found by polling launch_plan()["math"]."""
        if getattr(self, "_routed_warned", False):
            return
        if self.launch_plan(num_rows=1)["route"] == _lib.ROUTE_KEPT_FAST:
            # the other side of the same rule: the scene wants STRICT, the job is too deep for it
            self._routed_warned = True
            import warnings
            warnings.warn("flux_amd: this scene has a plane stored with a non-unit normal, but max_trace_depth leaves no room for the "
                          "STRICT arithmetic's recursion stack (31 levels of LDS, fewer with a mesh): the job stays on FLUX_MATH_FAST "
                          "with long-form glossy weights, and pixels the reference renders as NaN may come out finite. Normalise the "
                          "plane normals or lower max_trace_depth.", RuntimeWarning, stacklevel=3)
            return
        if self.requested_math == _lib.MATH_FAST and self.effective_math() == _lib.MATH_STRICT:
            self._routed_warned = True
            import warnings
            warnings.warn("flux_amd: this scene has a plane stored with a non-unit normal, so FLUX_MATH_FAST renders it with the STRICT "
                          "arithmetic (the reference's operation order, incl. its NaN pixels): several times slower. Normalise the "
                          "plane normals to get the FAST kernels.", RuntimeWarning, stacklevel=3)

    requested_math = _lib.MATH_FAST

    def effective_math(self) -> int:
        """The arithmetic a render really runs with (flux_ctx_launch_plan word 5)."""
        return self.launch_plan(num_rows=1)["math"]

    def __repr__(self):
        names = {_lib.MATH_FAST: "FAST", _lib.MATH_STRICT: "STRICT"}
        try:
            eff = self.effective_math()
            math = names[self.requested_math] + ("" if eff == self.requested_math else f" -> {names[eff]} (non-unit plane normal)")
        except Exception:
            math = "closed"
        return (f"Renderer({self.scene_data.scene_name!r}, {self.width}x{self.height}, sample_root {self.config.sample_root}, "
                f"depth {self.config.max_trace_depth}, seed {self.seed}, device {self.device}, math {math})")

    # -- lifetime ------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            _lib.lib.flux_ctx_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if not self._h:
            raise _lib.FluxError(_lib.E_INVALID, "renderer is closed")
        return self._h

    # -- Camera::render --------------------------------------------------------
    def render(self, unit: WorkUnit) -> WorkUnitResult:
        """Camera::render (trace.rs:53-97): rows [row_start,row_end] inclusive."""
        rows = self.render_rows(unit.row_start, unit.row_end)
        return WorkUnitResult(work_unit=unit, rows=rows)

    def _row_end(self, row_start, row_end):
        """the last row of [row_start, row_end] inclusive (None: the frame's last), the range checked"""
        if row_end is None:
            row_end = self.height - 1
        if row_start < 0 or row_end < row_start:
            raise _lib.FluxError(_lib.E_INVALID, f"bad row range [{row_start},{row_end}]")
        return row_end

    def render_rows(self, row_start: int, row_end: int) -> np.ndarray:
        row_end = self._row_end(row_start, row_end)
        out = np.empty((row_end - row_start + 1, self.width, 3), dtype=np.float64)
        _lib.check(_lib.lib.flux_render_rows(self._handle(), row_start, row_end,
                                             out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def render_rows_device(self, first_row: int, row_stride: int, num_rows: int, d_out_ptr: int, stream: int = 0):
        """Asynchronous device-resident render (see flux_render_rows_device)."""
        _lib.check(_lib.lib.flux_render_rows_device(self._handle(), first_row, row_stride, num_rows,
                                                    C.c_void_p(d_out_ptr), C.c_void_p(stream)))

    def render_sets_device(self, first_set: int, set_stride: int, num_sets: int, d_out_ptr: int, stream: int = 0):
        """Asynchronous device-resident render of the pixels whose sample set is first_set + m*set_stride
        (see flux_render_sets_device): out[(row*num_sets + m)*3]."""
        _lib.check(_lib.lib.flux_render_sets_device(self._handle(), first_set, set_stride, num_sets,
                                                    C.c_void_p(d_out_ptr), C.c_void_p(stream)))

    # -- first-hit feature buffers ---------------------------------------------
    def render_aov(self, row_start: int = 0, row_end=None) -> np.ndarray:
        """Albedo, normal, depth and coverage of rows [row_start, row_end] inclusive (default: the frame), [rows, W, 8]:
        flux_render_aov_rows.  Channels: flux_amd.AOV_ALBEDO, AOV_NORMAL (slices), AOV_DEPTH, AOV_COVERAGE."""
        row_end = self._row_end(row_start, row_end)
        out = np.empty((row_end - row_start + 1, self.width, _lib.AOV_CHANNELS), dtype=np.float64)
        _lib.check(_lib.lib.flux_render_aov_rows(self._handle(), row_start, row_end, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def render_aov_device(self, first_row: int, row_stride: int, num_rows: int, d_out_ptr: int, stream: int = 0):
        """Asynchronous device-resident feature buffers (see flux_render_aov_rows_device): num_rows * W * 8 doubles."""
        _lib.check(_lib.lib.flux_render_aov_rows_device(self._handle(), first_row, row_stride, num_rows,
                                                        C.c_void_p(d_out_ptr), C.c_void_p(stream)))

    # -- feature buffers at the first non-specular hit ---------------------------
    def render_aov_chain(self, max_chain: int = 0, row_start: int = 0, row_end=None) -> np.ndarray:
        """render_aov()'s buffers taken where each sample's chain of Reflective / Dielectric bounces ends, [rows, W, 8]:
        flux_render_aov_chain_rows.  max_chain: the most segments a chain has (0: max_trace_depth; 1 is render_aov() bit for bit)."""
        row_end = self._row_end(row_start, row_end)
        self._check_max_chain(max_chain)
        out = np.empty((row_end - row_start + 1, self.width, _lib.AOV_CHANNELS), dtype=np.float64)
        _lib.check(_lib.lib.flux_render_aov_chain_rows(self._handle(), row_start, row_end, max_chain,
                                                       out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    @staticmethod
    def _check_max_chain(max_chain):
        # (the parameter is a uint32_t: ctypes would wrap 2**32 to 0, which means the full depth)
        if not 0 <= int(max_chain) <= 0xFFFFFFFF:
            raise _lib.FluxError(_lib.E_INVALID, f"max_chain {max_chain} is outside 0 .. 2**32 - 1 (0 means max_trace_depth)")

    def render_aov_chain_device(self, first_row: int, row_stride: int, num_rows: int, d_out_ptr: int, max_chain: int = 0,
                                stream: int = 0):
        """Asynchronous device-resident form (see flux_render_aov_chain_rows_device): num_rows * W * 8 doubles."""
        self._check_max_chain(max_chain)
        _lib.check(_lib.lib.flux_render_aov_chain_rows_device(self._handle(), first_row, row_stride, num_rows, max_chain,
                                                              C.c_void_p(d_out_ptr), C.c_void_p(stream)))

    # -- per-pixel sample moments ------------------------------------------------
    def render_moments(self, row_start: int = 0, row_end=None) -> np.ndarray:
        """The frame and its measured variance for rows [row_start, row_end] inclusive (default: the frame), [rows, W, 8]:
        flux_render_moments_rows.  Channels: flux_amd.MOMENT_RGB (the frame), MOMENT_VAR, MOMENT_MEAN (unclamped), MOMENT_S2."""
        row_end = self._row_end(row_start, row_end)
        out = np.empty((row_end - row_start + 1, self.width, _lib.MOMENT_CHANNELS), dtype=np.float64)
        _lib.check(_lib.lib.flux_render_moments_rows(self._handle(), row_start, row_end, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def render_moments_device(self, first_row: int, row_stride: int, num_rows: int, d_out_ptr: int, stream: int = 0):
        """Asynchronous device-resident sample moments (see flux_render_moments_rows_device): num_rows * W * 8 doubles."""
        _lib.check(_lib.lib.flux_render_moments_rows_device(self._handle(), first_row, row_stride, num_rows,
                                                            C.c_void_p(d_out_ptr), C.c_void_p(stream)))

    # -- adaptive sampling ---------------------------------------------------------
    last_adaptive_info = None

    @staticmethod
    def _adaptive_params(threshold, max_passes, min_passes, lum_floor, dilate):
        return _lib.FluxAdaptiveParams(float(threshold), float(lum_floor), int(min_passes), int(max_passes), int(dilate), 0)

    def _keep_adaptive_info(self, info):
        self.last_adaptive_info = {"rounds": int(info[0]), "pixel_passes": int(info[1]), "pixels_at_max_passes": int(info[2]),
                                   "samples": int(info[1]) * self.config.sample_root ** 2}

    def render_adaptive(self, threshold: float = _lib.ADAPTIVE_THRESHOLD, max_passes: int = _lib.ADAPTIVE_MAX_PASSES,
                        min_passes: int = _lib.ADAPTIVE_MIN_PASSES, lum_floor: float = _lib.ADAPTIVE_LUM_FLOOR,
                        dilate: int = _lib.ADAPTIVE_DILATE, row_start: int = 0, row_end=None):
        """Adaptive sampling of rows [row_start, row_end] inclusive (default: the frame), flux_render_adaptive_rows: passes of one
        sample set (sample_root² samples) each, every pixel for `min_passes`, then only the pixels whose relative standard error
        exceeds `threshold` and their neighbours within `dilate`, up to `max_passes` (at most the image width).  Returns
        (moments [rows, W, 8], passes [rows, W] uint32): the layout of render_moments() with each pixel's own sample count behind
        its mean and variance, so flux_amd.denoise_moments(moments, r.render_aov()) filters an adaptive frame with its per-pixel
        variance, and no further denoiser call exists.  With max_passes=1 the moments are render_moments() bit for bit.
        last_adaptive_info holds the call's rounds, pixel passes, samples and pixels that reached max_passes."""
        row_end = self._row_end(row_start, row_end)
        rows = row_end - row_start + 1
        mom = np.empty((rows, self.width, _lib.MOMENT_CHANNELS), dtype=np.float64)
        passes = np.empty((rows, self.width), dtype=np.uint32)
        par = self._adaptive_params(threshold, max_passes, min_passes, lum_floor, dilate)
        info = (C.c_uint64 * _lib.ADAPTIVE_INFO_WORDS)()
        _lib.check(_lib.lib.flux_render_adaptive_rows(self._handle(), row_start, row_end, C.byref(par),
                                                      mom.ctypes.data_as(C.POINTER(C.c_double)), passes.ctypes.data_as(C.c_void_p), info))
        self._keep_adaptive_info(info)
        return mom, passes

    def render_adaptive_device(self, first_row: int, row_stride: int, num_rows: int, d_out_moments_ptr: int, d_out_passes_ptr: int,
                               threshold: float = _lib.ADAPTIVE_THRESHOLD, max_passes: int = _lib.ADAPTIVE_MAX_PASSES,
                               min_passes: int = _lib.ADAPTIVE_MIN_PASSES, lum_floor: float = _lib.ADAPTIVE_LUM_FLOOR,
                               dilate: int = _lib.ADAPTIVE_DILATE, stream: int = 0):
        """Device-resident adaptive sampling (see flux_render_adaptive_rows_device): num_rows * W * 8 doubles and num_rows * W
        uint32 on `stream`, which the call synchronises once per selective round.  Sets last_adaptive_info."""
        par = self._adaptive_params(threshold, max_passes, min_passes, lum_floor, dilate)
        info = (C.c_uint64 * _lib.ADAPTIVE_INFO_WORDS)()
        _lib.check(_lib.lib.flux_render_adaptive_rows_device(self._handle(), first_row, row_stride, num_rows, C.byref(par),
                                                             C.c_void_p(d_out_moments_ptr), C.c_void_p(d_out_passes_ptr), info,
                                                             C.c_void_p(stream)))
        self._keep_adaptive_info(info)

    def render_denoised(self, variance: str = "spatial", guides: str = "first", **params) -> np.ndarray:
        """The denoised frame on this renderer's device; `params` are flux_amd.denoise's.  variance="spatial" (the default):
        render_frame() + render_aov() + flux_amd.denoise, which estimates the noise from the frame.  variance="measured":
        render_moments() + render_aov() + flux_amd.denoise_moments -- one render, whose per-sample variance guides the filter.
        guides="first" (the default): render_aov(); guides="chain": render_aov_chain(), the features behind mirrors and glass."""
        if guides not in ("first", "chain"):
            raise _lib.FluxError(_lib.E_INVALID, f"render_denoised: guides must be 'first' or 'chain', got {guides!r}")
        if variance not in ("spatial", "measured"):
            raise _lib.FluxError(_lib.E_INVALID, f"render_denoised: variance must be 'spatial' or 'measured', got {variance!r}")
        frame = self.render_frame() if variance == "spatial" else self.render_moments()
        aov = self.render_aov() if guides == "first" else self.render_aov_chain()
        if variance == "spatial":
            return denoise(frame, aov, device=self.device, **params)
        return denoise_moments(frame, aov, device=self.device, **params)

    def debug_shade(self, origins, directions, depth: int = 1, set_index: int = 0, sample_index: int = 0):
        """Scene::shade on the device for the given rays (flux_debug_shade): (rgb [n,3], first-hit index [n], t [n])."""
        o = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
        d = np.ascontiguousarray(directions, dtype=np.float64).reshape(-1, 3)
        assert o.shape == d.shape
        rays = np.ascontiguousarray(np.concatenate([o, d], axis=1))
        n = rays.shape[0]
        rgb = np.empty((n, 3), dtype=np.float64)
        hit = np.empty(n, dtype=np.int32)
        t = np.empty(n, dtype=np.float64)
        dp = C.POINTER(C.c_double)
        _lib.check(_lib.lib.flux_debug_shade(self._handle(), n, rays.ctypes.data_as(dp), depth, set_index, sample_index,
                                             rgb.ctypes.data_as(dp), hit.ctypes.data_as(C.POINTER(C.c_int32)),
                                             t.ctypes.data_as(dp)))
        return rgb, hit, t

    def row_perm_table(self) -> np.ndarray:
        """[H][S] int32: the sample-set index of every pixel (row, col)."""
        return np.stack([self.row_perm(r) for r in range(self.height)])

    def render_frame(self) -> np.ndarray:
        return self.render_rows(0, self.height - 1)

    # -- knobs / introspection ---------------------------------------------------
    def set_kernel(self, variant: int):
        _lib.check(_lib.lib.flux_ctx_set_kernel(self._handle(), variant))

    def set_math(self, mode: int):
        """MATH_FAST (default) or MATH_STRICT (reference operation order); include/flux_abi.h."""
        _lib.check(_lib.lib.flux_ctx_set_math(self._handle(), mode))
        self.requested_math = int(mode)
        self._warn_if_routed()

    def last_kernel_ms(self) -> float:
        return float(_lib.lib.flux_ctx_last_kernel_ms(self._handle()))

    def enable_stats(self, on=True):
        _lib.check(_lib.lib.flux_ctx_enable_stats(self._handle(), 1 if on else 0))

    def stats(self, reset=False) -> dict:
        buf = (C.c_uint64 * _lib.NUM_STATS)()
        _lib.check(_lib.lib.flux_ctx_stats(self._handle(), buf, 1 if reset else 0))
        return dict(zip(STAT_NAMES, [int(x) for x in buf]))

    def stats_raw(self) -> list:
        """All FLUX_NUM_STATS slots (10 and 11 count dielectric bounces, 12.. are reserved: 0 in the product build;
        experiment builds with -DFLUX_DEBUG_TRIPS count loop trips in 10.., scripts/trip_counts.py)."""
        buf = (C.c_uint64 * _lib.NUM_STATS)()
        _lib.check(_lib.lib.flux_ctx_stats(self._handle(), buf, 0))
        return [int(x) for x in buf]

    def set_traversal(self, mode: int):
        """Extension: 0 = BVH (default), 1 = brute force over the triangles."""
        _lib.check(_lib.lib.flux_ctx_set_traversal(self._handle(), mode))

    def set_mesh_normals(self, mesh_index: int, normals):
        """Extension: smooth shading for mesh `mesh_index` (in the order of the scene's meshes) -- `normals` as MeshData.normals,
        [vertices][3] or [triangles][3][3]; None: back to the facet normals (flux_ctx_set_mesh_normals)."""
        self._set_mesh_attribute("normals", mesh_index, normals)

    def set_mesh_colors(self, mesh_index: int, colors):
        """Extension: vertex colours for mesh `mesh_index` (in the order of the scene's meshes) -- `colors` as MeshData.colors,
        [vertices][3] or [triangles][3][3]; None: the material's colour alone again (flux_ctx_set_mesh_colors)."""
        self._set_mesh_attribute("colors", mesh_index, colors)

    def _set_mesh_attribute(self, attr, mesh_index, values):
        meshes = split_shapes(self.scene_data)[1]
        if values is not None and 0 <= mesh_index < len(meshes):
            import dataclasses
            values = _corner_attribute(dataclasses.replace(meshes[mesh_index], **{attr: values}), attr, f"mesh {mesh_index}")
        _set_mesh_attribute(self._handle(), attr, mesh_index, values)

    def bvh_info(self) -> dict:
        buf = (C.c_uint64 * _lib.BVH_INFO_WORDS)()
        _lib.check(_lib.lib.flux_ctx_bvh_info(self._handle(), buf, _lib.BVH_INFO_WORDS))
        names = ("nodes", "triangles", "max_depth", "max_leaf", "node_bytes", "tri_bytes", "build_us", "wide_nodes",
                 "leaf_records", "fused_leaves", "wide_stack", "wide_node_bytes", "leaf_record_bytes", "wide_in_use")
        return dict(zip(names, [int(x) for x in buf]))

    def launch_plan(self, num_rows=None, num_sets: int = 0, flags: bool = False) -> dict:
        """What a render call would launch with the current settings (flux_ctx_launch_plan: the library's own launch
        planner): `num_rows` rows of all sets (flux_render_rows*), or `num_sets` of this context's sets over all rows
        (flux_render_sets_device) when num_sets > 0.  `flags`: the dict also holds "flags", the instantiation of the kernel
        (_lib.PLAN_FLAG_*, word 7).  On request only: the other words say what is launched and stay equal under the switches that
        take one choice of the instantiation away (FLUX_PLANE_AXIS=0, FLUX_THROUGHPUT_TABLE=0, ...), which callers compare plans by."""
        buf = (C.c_int64 * _lib.PLAN_WORDS)()
        _lib.check(_lib.lib.flux_ctx_launch_plan(self._handle(), self.height if num_rows is None else num_rows, num_sets, buf))
        names = ("kernel", "block", "blocks", "lds", "waves_per_pixel", "math", "route") + (("flags",) if flags else ())
        return dict(zip(names, [int(x) for x in buf]))

    def table(self, which: int) -> np.ndarray:
        S = len(range(self.set_share[0], self.width, self.set_share[1]))  # the sets held, in slot order
        N = self.config.sample_root ** 2
        D = self.config.max_trace_depth
        shape = (S, N, 2) if which in (_lib.TABLE_PIXEL, _lib.TABLE_DISC) else (S, N) if which == _lib.TABLE_ORDER else (S, D, N, 3)
        out = np.empty(shape, dtype=np.float64)
        _lib.check(_lib.lib.flux_ctx_copy_table(self._handle(), which, out.ctypes.data_as(C.POINTER(C.c_double)),
                                                out.size))
        return out

    def row_perm(self, row: int) -> np.ndarray:
        out = np.empty(self.width, dtype=np.int32)
        _lib.check(_lib.lib.flux_ctx_copy_row_perm(self._handle(), row, out.ctypes.data_as(C.POINTER(C.c_int32)),
                                                   out.size))
        return out

    def camera_basis(self) -> np.ndarray:
        out = np.empty(9, dtype=np.float64)
        _lib.check(_lib.lib.flux_ctx_camera_basis(self._handle(), out.ctypes.data_as(C.POINTER(C.c_double))))
        return out.reshape(3, 3)

    def device_bytes(self) -> int:
        return int(_lib.lib.flux_ctx_device_bytes(self._handle()))

    def create_timing(self) -> dict:
        """Where the wall time of this context's creation went, in ms (flux_ctx_create_timing): total, host, runtime,
        alloc, upload, tables, free, other -- the span the reference's timer includes (manager.rs:145 -> 170)."""
        return _create_timing(self._handle())


def _set_mesh_attribute(handle, attr, mesh_index, corners):
    """the attribute's call (MESH_ATTRIBUTES[attr].setter): `corners` [nt][3][3] float64, or None to clear"""
    setter = getattr(_lib.lib, MESH_ATTRIBUTES[attr].setter)
    if mesh_index < 0:
        raise _lib.FluxError(_lib.E_INVALID, f"mesh index {mesh_index} out of range")
    if corners is None:
        _lib.check(setter(handle, mesh_index, None, 0))
        return
    c = np.ascontiguousarray(corners, dtype=np.float64)
    _lib.check(setter(handle, mesh_index, c.ctypes.data_as(C.POINTER(C.c_double)), c.size // 9))


def _set_scene_attributes(handle, scene_data):
    """every attribute of every mesh of the scene that has it, on one context: the normals of all meshes, then the colours"""
    for attr in MESH_ATTRIBUTES:
        for i, m in enumerate(split_shapes(scene_data)[1]):
            corners = _corner_attribute(m, attr, f"mesh {i}")
            if corners is not None and len(corners):
                _set_mesh_attribute(handle, attr, i, corners)


def _create_timing(handle) -> dict:
    buf = (C.c_double * _lib.CREATE_TIMING_WORDS)()
    _lib.check(_lib.lib.flux_ctx_create_timing(handle, buf))
    return dict(zip(_lib.CREATE_TIMING_NAMES, [float(x) for x in buf]))


class MultiRenderer:
    """One frame on several GPUs of THIS process through the C ABI (flux_multi_*): the job's fan-out to its workers
    (fluxcore/src/manager.rs:156-162) as one context per device, each holding its share of the sample tables, and ImageBuilder's
    gather (manager.rs:316-324) as ONE ncclAllGather (RCCL) + a reassembly kernel on devices[0].  No torch.distributed."""

    def __init__(self, scene_data: SceneData, config: JobConfiguration, seed: int = 1, devices=(0,), shard: int = _lib.SHARD_AUTO):
        self.scene_data, self.config, self.seed = scene_data, config, int(seed)
        self.devices = [int(d) for d in devices]
        self.width = scene_data.output_settings.image_width
        self.height = scene_data.output_settings.image_height
        self._desc = SceneDesc(scene_data)
        cfg = _lib.FluxJobCfg(config.sample_root, config.max_trace_depth, config.rows_per_work_unit)
        devs = (C.c_int * len(self.devices))(*self.devices)
        h = C.c_void_p()
        _lib.check(_lib.lib.flux_multi_create(C.byref(self._desc.desc), C.byref(cfg), C.c_uint64(self.seed), devs, len(self.devices),
                                              int(shard), C.byref(h)))
        self._h = h
        for rank in range(len(self.devices)):  # every rank's context gets the meshes' normals and colours
            ctx = C.c_void_p()
            _lib.check(_lib.lib.flux_multi_ctx(h, rank, C.byref(ctx)))
            _set_scene_attributes(ctx, scene_data)

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib.flux_multi_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if not self._h:
            raise _lib.FluxError(_lib.E_INVALID, "multi renderer is closed")
        return self._h

    def render_frame(self) -> np.ndarray:
        out = np.empty((self.height, self.width, 3), dtype=np.float64)
        _lib.check(_lib.lib.flux_multi_render_frame(self._handle(), out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def render_frame_device(self) -> int:
        """The frame left on devices[0]: its device address ([H][W][3] f64), valid until the next render call."""
        p = C.c_void_p()
        _lib.check(_lib.lib.flux_multi_render_frame_device(self._handle(), C.byref(p)))
        return int(p.value)

    def set_kernel(self, variant: int):
        _lib.check(_lib.lib.flux_multi_set_kernel(self._handle(), variant))

    def set_math(self, mode: int):
        _lib.check(_lib.lib.flux_multi_set_math(self._handle(), mode))

    def info(self) -> dict:
        buf = (C.c_uint64 * _lib.MULTI_INFO_WORDS)()
        _lib.check(_lib.lib.flux_multi_info(self._handle(), buf))
        names = ("devices", "shard", "rccl_version", "share_doubles", "ctx_bytes", "buffer_bytes", "comms_cached")
        return dict(zip(names, [int(x) for x in buf]))

    def timing(self) -> dict:
        buf = (C.c_double * _lib.MULTI_TIMING_WORDS)()
        _lib.check(_lib.lib.flux_multi_timing(self._handle(), buf))
        names = ("create_ms", "ctx_create_ms", "comm_init_ms", "frame_ms", "kernel_ms", "all_gather_ms", "reassembly_ms", "d2h_ms")
        return dict(zip(names, [float(x) for x in buf]))

    def rank_create_timing(self, rank: int = 0) -> dict:
        h = C.c_void_p()
        _lib.check(_lib.lib.flux_multi_ctx(self._handle(), rank, C.byref(h)))
        return _create_timing(h)

    def rank_renderer(self, rank: int = 0) -> "Renderer":
        """Rank's context as a Renderer (BORROWED: flux_multi_ctx; closing it does nothing) -- for launch_plan, statistics, tables."""
        h = C.c_void_p()
        _lib.check(_lib.lib.flux_multi_ctx(self._handle(), rank, C.byref(h)))
        r = _BorrowedRenderer.__new__(_BorrowedRenderer)
        r.scene_data, r.config, r.seed, r.device = self.scene_data, self.config, self.seed, self.devices[rank]
        r.width, r.height = self.width, self.height
        info = self.info()
        r.set_share = (rank, len(self.devices)) if info["shard"] == _lib.SHARD_SETS else (0, 1)
        r._h = h
        r._routed_warned = True
        return r


class _BorrowedRenderer(Renderer):
    def close(self):
        self._h = None


def render_frame_multi(scene_data: SceneData, config: JobConfiguration, seed: int = 1, num_devices: int = 0,
                       shard: int = _lib.SHARD_AUTO) -> np.ndarray:
    """flux_render_frame_multi: create + render + destroy on the first `num_devices` devices (0 = all).  The one call has no place
    for mesh attributes (their calls work on a context), so a scene with a smooth or coloured mesh is refused: use MultiRenderer."""
    for attr, row in MESH_ATTRIBUTES.items():
        if any(getattr(m, attr) is not None for m in split_shapes(scene_data)[1]):
            raise _lib.FluxError(_lib.E_INVALID, row.multi_refusal)
    desc = SceneDesc(scene_data)
    cfg = _lib.FluxJobCfg(config.sample_root, config.max_trace_depth, config.rows_per_work_unit)
    out = np.empty((scene_data.output_settings.image_height, scene_data.output_settings.image_width, 3), dtype=np.float64)
    _lib.check(_lib.lib.flux_render_frame_multi(C.byref(desc.desc), C.byref(cfg), C.c_uint64(int(seed)), None, num_devices, int(shard),
                                                out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def release_comms() -> int:
    return int(_lib.lib.flux_multi_release_comms())


def work_units(image_height: int, rows_per_work_unit: int):
    """Job::work_units (job.rs:65-88) through the C ABI."""
    n = _lib.lib.flux_work_units(image_height, rows_per_work_unit, None, 0)
    _lib.check(n)
    buf = (_lib.FluxWorkUnit * max(n, 1))()
    _lib.check(_lib.lib.flux_work_units(image_height, rows_per_work_unit, buf, n))
    return [WorkUnit(int(buf[i].row_start), int(buf[i].row_end)) for i in range(n)]


def write_ppm(path: str, rgb: np.ndarray, rows_present=None):
    """Image::write (image.rs:43-61) through the C ABI."""
    rgb = np.ascontiguousarray(rgb, dtype=np.float64)
    h, w, c = rgb.shape
    assert c == 3
    rp = None
    if rows_present is not None:
        rp_arr = np.ascontiguousarray(rows_present, dtype=np.uint8)
        assert rp_arr.shape == (h,)
        rp = rp_arr.ctypes.data_as(C.POINTER(C.c_uint8))
    _lib.check(_lib.lib.flux_write_ppm(path.encode(), rgb.ctypes.data_as(C.POINTER(C.c_double)), w, h, rp))


def _denoise_params(levels, sigma_l, sigma_n, sigma_z, sigma_a):
    """The FLUX_DENOISE_PARAM_WORDS doubles of flux_denoise (the library checks their ranges)."""
    return (C.c_double * _lib.DENOISE_PARAM_WORDS)(levels, sigma_l, sigma_n, sigma_z, sigma_a, 0.0, 0.0, 0.0)


def _denoise_host(name, what, channels, x, aov, device, params):
    """denoise and denoise_moments as `name`: flux_<name> over the input `x` [H, W, channels], which the error text calls `what`."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    aov = np.ascontiguousarray(aov, dtype=np.float64)
    if x.ndim != 3 or x.shape[2] != channels or aov.shape != x.shape[:2] + (_lib.AOV_CHANNELS,):
        raise _lib.FluxError(_lib.E_INVALID, f"{name}: {what} {x.shape} and aov {aov.shape} are not "
                                             f"[H, W, {channels}] and [H, W, {_lib.AOV_CHANNELS}]")
    out = np.empty(x.shape[:2] + (3,), dtype=np.float64)
    dp = C.POINTER(C.c_double)
    _lib.check(getattr(_lib.lib, "flux_" + name)(int(device), x.shape[1], x.shape[0], x.ctypes.data_as(dp), aov.ctypes.data_as(dp), params,
                                                 out.ctypes.data_as(dp)))
    return out


def _denoise_device(name, width, height, d_in_ptr, d_aov_ptr, d_out_ptr, d_work_ptr, work_doubles, stream, device, params):
    """denoise_device and denoise_moments_device as `name`: flux_<name> on device addresses."""
    _lib.check(getattr(_lib.lib, "flux_" + name)(int(device), width, height, C.c_void_p(d_in_ptr), C.c_void_p(d_aov_ptr), params,
                                                 C.c_void_p(d_out_ptr), C.c_void_p(d_work_ptr), work_doubles, C.c_void_p(stream)))


def denoise(rgb, aov, device: int = 0, levels=5, sigma_l=2.0, sigma_n=0.35, sigma_z=0.1, sigma_a=0.1) -> np.ndarray:
    """The feature-guided a-trous filter of flux_denoise (include/flux_abi.h) over a frame `rgb` [H, W, 3] of
    render_frame() and its feature buffers `aov` [H, W, 8] of render_aov(): the filtered frame, on `device`.  Meant for noisy
    previews (1-16 spp); a frame that is already clean can come out worse."""
    return _denoise_host("denoise", "rgb", 3, rgb, aov, device, _denoise_params(levels, sigma_l, sigma_n, sigma_z, sigma_a))


def denoise_work_doubles(width: int, height: int) -> int:
    """Doubles of device scratch denoise_device needs (flux_denoise_work_doubles; 0 for a size the filter refuses)."""
    return int(_lib.lib.flux_denoise_work_doubles(width, height))


def denoise_device(width: int, height: int, d_rgb_ptr: int, d_aov_ptr: int, d_out_ptr: int, d_work_ptr: int, work_doubles: int,
                   stream: int = 0, device: int = 0, levels=5, sigma_l=2.0, sigma_n=0.35, sigma_z=0.1, sigma_a=0.1):
    """Asynchronous device-resident filter (see flux_denoise_device): device addresses of the frame, the feature buffers, the
    output frame and `work_doubles` >= denoise_work_doubles(width, height) doubles of scratch; `stream` a hipStream_t."""
    _denoise_device("denoise_device", width, height, d_rgb_ptr, d_aov_ptr, d_out_ptr, d_work_ptr, work_doubles, stream, device,
                    _denoise_params(levels, sigma_l, sigma_n, sigma_z, sigma_a))


def denoise_moments(moments, aov, device: int = 0, levels=5, sigma_l=2.0, sigma_n=0.35, sigma_z=0.1, sigma_a=0.1) -> np.ndarray:
    """flux_denoise_moments (include/flux_abi.h): the a-trous filter of `denoise` guided by the measured
    variance -- `moments` [H, W, 8] of render_moments(), whose channels 0..2 are the frame and channel 3 its variance, and `aov`
    [H, W, 8] of render_aov(): the filtered frame [H, W, 3], on `device`."""
    return _denoise_host("denoise_moments", "moments", _lib.MOMENT_CHANNELS, moments, aov, device,
                         _denoise_params(levels, sigma_l, sigma_n, sigma_z, sigma_a))


def denoise_moments_device(width: int, height: int, d_moments_ptr: int, d_aov_ptr: int, d_out_ptr: int, d_work_ptr: int,
                           work_doubles: int, stream: int = 0, device: int = 0, levels=5, sigma_l=2.0, sigma_n=0.35, sigma_z=0.1,
                           sigma_a=0.1):
    """Asynchronous device-resident filter (see flux_denoise_moments_device): device addresses of the moments, the feature buffers,
    the output frame and `work_doubles` >= denoise_work_doubles(width, height) doubles of scratch; `stream` a hipStream_t."""
    _denoise_device("denoise_moments_device", width, height, d_moments_ptr, d_aov_ptr, d_out_ptr, d_work_ptr, work_doubles, stream, device,
                    _denoise_params(levels, sigma_l, sigma_n, sigma_z, sigma_a))


def debug_fastmath(fn: int, a, b=None, device: int = 0) -> np.ndarray:
    """out[i] = fn(a[i], b[i]) evaluated on the device by csrc/flux_math.h (test hook)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    out = np.empty_like(a)
    pa = a.ctypes.data_as(C.POINTER(C.c_double))
    pb = None
    if b is not None:
        b = np.ascontiguousarray(b, dtype=np.float64)
        assert b.shape == a.shape
        pb = b.ctypes.data_as(C.POINTER(C.c_double))
    _lib.check(_lib.lib.flux_debug_fastmath(device, fn, pa, pb, out.ctypes.data_as(C.POINTER(C.c_double)), a.size))
    return out


def debug_plane_div(num, den, device: int = 0):
    """The split kernel's unscaled first-plane division, num / den and the votes' word on den, evaluated on the device by
    csrc/flux_plane_axis.h (test hook, include/flux_abi.h flux_debug_plane_div): (unscaled, quotient, admit)."""
    num = np.ascontiguousarray(num, dtype=np.float64)
    den = np.ascontiguousarray(den, dtype=np.float64)
    assert num.shape == den.shape
    unscaled, quotient, admit = np.empty_like(num), np.empty_like(num), np.empty(num.shape, dtype=np.int32)
    pd = C.POINTER(C.c_double)
    _lib.check(_lib.lib.flux_debug_plane_div(device, num.ctypes.data_as(pd), den.ctypes.data_as(pd), unscaled.ctypes.data_as(pd),
                                             quotient.ctypes.data_as(pd), admit.ctypes.data_as(C.POINTER(C.c_int32)), num.size))
    return unscaled, quotient, admit


def sampler_grid(kind: int, sample_root: int, seed: int = 1, hemi: bool = False, device: int = 0):
    """One set of a samplers-crate generator computed on the device (include/flux_abi.h flux_sampler_grid):
    (n*n, 2) array, plus its to_hemisphere(.., 0.0) image (n*n, 3) when hemi=True."""
    n2 = sample_root * sample_root
    xy = np.empty((n2, 2), dtype=np.float64)
    hm = np.empty((n2, 3), dtype=np.float64) if hemi else None
    _lib.check(_lib.lib.flux_sampler_grid(device, kind, sample_root, seed, xy.ctypes.data_as(C.POINTER(C.c_double)),
                                          hm.ctypes.data_as(C.POINTER(C.c_double)) if hemi else None))
    return (xy, hm) if hemi else xy
