"""Cost of the feature buffers at the first non-specular hit (flux_render_aov_chain_rows) against the first-hit
buffers and the sample moments of the same job on the same context: in one process, after a warm-up, the three calls alternate and
the median of flux_ctx_last_kernel_ms of each is reported.  FAST arithmetic.  Development aid, not the bench contract.
usage: aov_chain_time.py [reps]      jobs: glass and mirror_glass, 800 x 600, at 16 and 256 spp"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flux_amd  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
JOBS = [("glass", 4), ("glass", 16), ("mirror_glass", 4), ("mirror_glass", 16)]


def alternate(r):
    """(aov ms, chain ms, moments ms): medians of `reps` alternating calls after one warm-up of each."""
    calls = (r.render_aov, r.render_aov_chain, r.render_moments)
    for call in calls:
        call()
    ms = [[] for _ in calls]
    for _ in range(reps):
        for k, call in enumerate(calls):
            call()
            ms[k].append(r.last_kernel_ms())
    return [statistics.median(x) for x in ms]


for name, root in JOBS:
    sd = flux_amd.load_scene(os.path.join(ROOT, "scenes", name + ".yml"))
    with flux_amd.Renderer(sd, flux_amd.JobConfiguration(root, 5, 50), seed=1) as r:
        aov_ms, chain_ms, moments_ms = alternate(r)
    print(json.dumps({"scene": name, "spp": root * root, "reps": reps, "math": "fast", "aov_ms": round(aov_ms, 3),
                      "chain_ms": round(chain_ms, 3), "moments_ms": round(moments_ms, 3), "chain_over_aov": round(chain_ms / aov_ms, 3),
                      "chain_over_moments": round(chain_ms / moments_ms, 4), "chain_below_moments": chain_ms < moments_ms}), flush=True)
