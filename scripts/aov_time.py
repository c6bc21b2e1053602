"""Cost of the first-hit feature buffers (flux_render_aov_rows) against the render of the same job on the
same context: in one process, after a warm-up, the two calls alternate and the median of flux_ctx_last_kernel_ms of each is
reported; then the same for a context of the job at max_trace_depth 1.  Development aid, not the bench contract.
usage: aov_time.py [reps]      jobs: demo2 800 x 600 at 256 and 16384 spp, the 1M-triangle height field of bench.py --config 5 at 256 spp"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flux_amd  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
JOBS = [("demo2", 16), ("demo2", 128), ("hf:1000x500", 16)]


def scene(name):
    if name.startswith("hf:"):
        from flux_amd.procedural import heightfield_scene
        nx, nz = [int(x) for x in name[3:].split("x")]
        return heightfield_scene(nx, nz)
    return flux_amd.load_scene(os.path.join(ROOT, "scenes", name + ".yml"))


def alternate(r):
    """(render ms, aov ms): medians of `reps` alternating calls after one warm-up of each."""
    r.render_frame()
    r.render_aov()
    render, aov = [], []
    for _ in range(reps):
        r.render_frame()
        render.append(r.last_kernel_ms())
        r.render_aov()
        aov.append(r.last_kernel_ms())
    return statistics.median(render), statistics.median(aov)


for name, root in JOBS:
    sd = scene(name)
    out = {"scene": name, "spp": root * root, "reps": reps, "math": "fast"}
    for depth in (5, 1):
        with flux_amd.Renderer(sd, flux_amd.JobConfiguration(root, depth, 50), seed=1) as r:
            render_ms, aov_ms = alternate(r)
            out[f"depth{depth}"] = {"render_ms": round(render_ms, 3), "aov_ms": round(aov_ms, 3), "aov_over_render": round(aov_ms / render_ms, 4),
                                    "render_kernel": r.launch_plan()["kernel"]}
    out["aov_below_full_depth_render"] = out["depth5"]["aov_ms"] < out["depth5"]["render_ms"]
    print(json.dumps(out), flush=True)
