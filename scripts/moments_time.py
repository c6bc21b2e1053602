"""Cost of the per-pixel sample moments (flux_render_moments_rows) against the render of the same job on the
same context -- under FLUX_KERNEL_STATIC, whose loop the moments kernel shares, and under the default kernel: in one process, after a
warm-up, the three calls alternate and the median of flux_ctx_last_kernel_ms of each is reported.  Then flux_denoise_moments_device
against flux_denoise_device on demo2 at 800 x 600, 16 spp, with device events around the launches, alternating.
Development aid, not the bench contract.
usage: moments_time.py [reps]      jobs: demo2 800 x 600 at 16 and 256 spp, the 1M-triangle height field of bench.py --config 5 at 256 spp"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import flux_amd  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
JOBS = [("demo2", 4), ("demo2", 16), ("hf:1000x500", 16)]


def scene(name):
    if name.startswith("hf:"):
        from flux_amd.procedural import heightfield_scene
        nx, nz = [int(x) for x in name[3:].split("x")]
        return heightfield_scene(nx, nz)
    return flux_amd.load_scene(os.path.join(ROOT, "scenes", name + ".yml"))


def alternate(r):
    """(static render ms, moments ms, default render ms): medians of `reps` alternating calls after one warm-up of each."""
    def static():
        r.set_kernel(flux_amd.KERNEL_STATIC)
        r.render_frame()

    def default():
        r.set_kernel(flux_amd.KERNEL_DEFAULT)
        r.render_frame()
    calls = (static, r.render_moments, default)
    for c in calls:
        c()
    ms = [[], [], []]
    for _ in range(reps):
        for k, c in enumerate(calls):
            c()
            ms[k].append(r.last_kernel_ms())
    plan = r.launch_plan()["kernel"]
    return [statistics.median(m) for m in ms], plan


frame_inputs = None
for name, root in JOBS:
    sd = scene(name)
    with flux_amd.Renderer(sd, flux_amd.JobConfiguration(root, 5, 50), seed=1) as r:
        (static_ms, moments_ms, default_ms), plan = alternate(r)
        if (name, root) == ("demo2", 4):
            frame_inputs = (r.render_frame(), r.render_moments(), r.render_aov())
    print(json.dumps({"scene": name, "spp": root * root, "reps": reps, "math": "fast", "static_render_ms": round(static_ms, 3),
                      "moments_ms": round(moments_ms, 3), "default_render_ms": round(default_ms, 3), "default_kernel": plan,
                      "moments_over_static": round(moments_ms / static_ms, 4), "moments_over_default": round(moments_ms / default_ms, 4)}),
          flush=True)

frame, mom, aov = frame_inputs
H, W, _ = frame.shape
dev = torch.device("cuda", 0)
d_rgb, d_mom, d_aov = (torch.from_numpy(a).to(dev) for a in (frame, mom, aov))
d_out = torch.empty_like(d_rgb)
need = flux_amd.denoise_work_doubles(W, H)
d_work = torch.empty(need, dtype=torch.float64, device=dev)
stream = torch.cuda.Stream(device=dev)
ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(fn, d_in):
    with torch.cuda.stream(stream):
        ev0.record(stream)
        fn(W, H, d_in.data_ptr(), d_aov.data_ptr(), d_out.data_ptr(), d_work.data_ptr(), need, stream=stream.cuda_stream)
        ev1.record(stream)
    stream.synchronize()
    return ev0.elapsed_time(ev1)


torch.cuda.synchronize()
timed(flux_amd.denoise_device, d_rgb)
timed(flux_amd.denoise_moments_device, d_mom)
spatial, measured = [], []
for _ in range(reps):
    spatial.append(timed(flux_amd.denoise_device, d_rgb))
    measured.append(timed(flux_amd.denoise_moments_device, d_mom))
print(json.dumps({"scene": "demo2", "size": [W, H], "spp": 16, "reps": reps, "denoise_ms": round(statistics.median(spatial), 3),
                  "denoise_moments_ms": round(statistics.median(measured), 3),
                  "measured_over_spatial": round(statistics.median(measured) / statistics.median(spatial), 4)}), flush=True)
