"""flux_amd -- MI355X (gfx950) implementation of jtdaugherty/flux's per-pixel render loop.

The package is a thin host layer over flux_amd/libflux_hip.so (hand-written HIP
kernels behind the C ABI of include/flux_abi.h).  Importing it without the
built library raises ImportError: there is no CPU fallback.
"""
from . import _lib
from ._lib import (AOV_ALBEDO, AOV_CHANNELS, AOV_COVERAGE, AOV_DEPTH, AOV_NORMAL, FluxError, KERNEL_DEFAULT, KERNEL_REFILL, KERNEL_SPLIT, KERNEL_STATIC, MATH_FAST, MATH_STRICT, SHARD_AUTO, SHARD_ROWS,
                   SHARD_SETS, ADAPTIVE_DILATE, ADAPTIVE_LUM_FLOOR, ADAPTIVE_MAX_PASSES, ADAPTIVE_MIN_PASSES, ADAPTIVE_THRESHOLD, MOMENT_CHANNELS, MOMENT_MEAN, MOMENT_RGB, MOMENT_S2, MOMENT_VAR)
from .render import MultiRenderer, Renderer, debug_fastmath, debug_plane_div, denoise, denoise_device, denoise_moments, denoise_moments_device, denoise_work_doubles, release_comms, render_frame_multi, sampler_grid, work_units, write_ppm
from .scene import (CameraData, CameraSettings, BoxData, DielectricData, DiskData, EmissiveData, GlossyReflectiveData, JobConfiguration, MatteData,
                    OutputSettings, PlaneData, ReflectiveData, SceneData, SceneError, SphereData, WorkUnit,
                    WorkUnitResult, load_scene, scene_from_dict)

__all__ = [
    "FluxError", "Renderer", "work_units", "write_ppm", "load_scene", "scene_from_dict", "SceneData", "SceneError",
    "CameraSettings", "CameraData", "OutputSettings", "SphereData", "PlaneData", "DiskData", "BoxData", "MatteData", "EmissiveData",
    "ReflectiveData", "GlossyReflectiveData", "DielectricData", "JobConfiguration", "WorkUnit", "WorkUnitResult", "KERNEL_DEFAULT",
    "KERNEL_STATIC", "KERNEL_REFILL", "KERNEL_SPLIT", "MATH_FAST", "MATH_STRICT", "debug_fastmath", "debug_plane_div", "sampler_grid",
    "MultiRenderer", "render_frame_multi", "release_comms", "SHARD_AUTO", "SHARD_SETS", "SHARD_ROWS",
    "AOV_ALBEDO", "AOV_NORMAL", "AOV_DEPTH", "AOV_COVERAGE", "AOV_CHANNELS", "denoise", "denoise_device", "denoise_work_doubles",
    "MOMENT_RGB", "MOMENT_VAR", "MOMENT_MEAN", "MOMENT_S2", "MOMENT_CHANNELS", "denoise_moments", "denoise_moments_device",
    "ADAPTIVE_THRESHOLD", "ADAPTIVE_LUM_FLOOR", "ADAPTIVE_MIN_PASSES", "ADAPTIVE_MAX_PASSES", "ADAPTIVE_DILATE",
]
