"""Cost of the a-trous denoiser (flux_denoise_device) against the render and the feature-buffer pass of the same
scene: in one process, after a warm-up, the median of `reps` runs of each.  The render and the feature buffers are timed by the
context's own events (flux_ctx_last_kernel_ms); the filter by device events around the launches of flux_denoise_device on a frame
and feature buffers that stay on the device.  Then the per-level split (the filter at 1 .. 5 levels: each difference is one more
level, the first figure holds the pack and variance kernels too) and the tiling A/B: the first n levels through LDS tiles
(FLUX_DENOISE_LDS_LEVELS = n), n = 0 .. 5 -- the difference of two neighbours is what level n - 1 gains or loses by it.
Development aid, not the bench contract.
usage: denoise_time.py [reps]      demo2 at 800 x 600"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import flux_amd  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
sd = flux_amd.load_scene(os.path.join(ROOT, "scenes", "demo2.yml"))
W, H = sd.output_settings.image_width, sd.output_settings.image_height
dev = torch.device("cuda", 0)


def median_ms(call, last_ms):
    call()
    out = []
    for _ in range(reps):
        call()
        out.append(last_ms())
    return statistics.median(out)


result = {"scene": "demo2", "size": [W, H], "reps": reps}
frame = aov = None
for root in (4, 16):
    with flux_amd.Renderer(sd, flux_amd.JobConfiguration(root, 5, 50), seed=1) as r:
        result[f"render_{root * root}spp_ms"] = round(median_ms(r.render_frame, r.last_kernel_ms), 3)
        result[f"aov_{root * root}spp_ms"] = round(median_ms(r.render_aov, r.last_kernel_ms), 3)
        if root == 4:
            frame, aov = r.render_frame(), r.render_aov()

d_rgb, d_aov = torch.from_numpy(frame).to(dev), torch.from_numpy(aov).to(dev)
d_out = torch.empty_like(d_rgb)
need = flux_amd.denoise_work_doubles(W, H)
d_work = torch.empty(need, dtype=torch.float64, device=dev)
stream = torch.cuda.Stream(device=dev)


def filter_ms(levels):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    state = {}

    def call():
        with torch.cuda.stream(stream):
            ev0.record(stream)
            flux_amd.denoise_device(W, H, d_rgb.data_ptr(), d_aov.data_ptr(), d_out.data_ptr(), d_work.data_ptr(), need,
                                    stream=stream.cuda_stream, levels=levels)
            ev1.record(stream)
        stream.synchronize()
        state["ms"] = ev0.elapsed_time(ev1)
    return median_ms(call, lambda: state["ms"])


torch.cuda.synchronize()
result["work_bytes"] = need * 8
os.environ["FLUX_DENOISE_LDS_LEVELS"] = "0"
result["gathers_by_levels_ms"] = {str(k): round(filter_ms(k), 3) for k in range(1, 6)}
result["lds_first_n_levels_ms"] = {}
for n in range(0, 6):
    os.environ["FLUX_DENOISE_LDS_LEVELS"] = str(n)
    result["lds_first_n_levels_ms"][str(n)] = round(filter_ms(5), 3)
os.environ.pop("FLUX_DENOISE_LDS_LEVELS", None)
result["denoise_ms"] = round(filter_ms(5), 3)  # the library's own choice of tiling, measured last: the device is warm
result["denoise_over_render_16spp"] = round(result["denoise_ms"] / result["render_16spp_ms"], 3)
result["denoise_over_render_256spp"] = round(result["denoise_ms"] / result["render_256spp_ms"], 3)
result["denoise_over_aov_16spp"] = round(result["denoise_ms"] / result["aov_16spp_ms"], 3)
print(json.dumps(result), flush=True)
