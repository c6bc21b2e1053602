"""Cost of adaptive sampling (flux_render_adaptive_rows) on demo2 at 800 x 600, FAST, in one process: after a
warm-up the calls alternate and the median of flux_ctx_last_kernel_ms of each is reported.
  per sample root (2 and 4): render_moments against render_adaptive with max_passes = 1 -- the difference is what the state and
      the finish kernel cost without any selection --, then a full adaptive frame at the default threshold with max_passes = 8: its
      rounds, mean samples per pixel, and its time per traced sample against the moments pass's;
  per uniform root given: the moments pass at that root, for the comparison with the uniform frame of the quality table.
Development aid, not the bench contract.
usage: adaptive_time.py [reps] [uniform roots ...]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flux_amd  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
uniform_roots = [int(x) for x in sys.argv[2:]]
sd = flux_amd.load_scene(os.path.join(ROOT, "scenes", "demo2.yml"))
W, H = sd.output_settings.image_width, sd.output_settings.image_height


def median_ms(r, calls):
    for c in calls:
        c()
    ms = [[] for _ in calls]
    for _ in range(reps):
        for k, c in enumerate(calls):
            c()
            ms[k].append(r.last_kernel_ms())
    return [statistics.median(m) for m in ms]


for root in (2, 4):
    N = root * root
    with flux_amd.Renderer(sd, flux_amd.JobConfiguration(root, 5, 50), seed=1) as r:
        moments_ms, one_ms, full_ms = median_ms(r, (r.render_moments, lambda: r.render_adaptive(max_passes=1), lambda: r.render_adaptive(max_passes=8)))
        info = r.last_adaptive_info
    spp = info["samples"] / (W * H)
    per_moments, per_adaptive = moments_ms / (W * H * N), full_ms / info["samples"]
    print(json.dumps({"scene": "demo2", "size": [W, H], "root": root, "reps": reps, "math": "fast", "moments_ms": round(moments_ms, 3),
                      "adaptive_one_pass_ms": round(one_ms, 3), "one_pass_over_moments": round(one_ms / moments_ms, 4),
                      "adaptive_ms": round(full_ms, 3), "threshold": flux_amd.ADAPTIVE_THRESHOLD, "max_passes": 8, "rounds": info["rounds"],
                      "samples_per_pixel": round(spp, 3), "pixels_at_max_passes": info["pixels_at_max_passes"],
                      "ns_per_sample_moments": round(per_moments * 1e6, 4), "ns_per_sample_adaptive": round(per_adaptive * 1e6, 4),
                      "adaptive_over_moments_per_sample": round(per_adaptive / per_moments, 4)}), flush=True)

for root in uniform_roots:
    with flux_amd.Renderer(sd, flux_amd.JobConfiguration(root, 5, 50), seed=1) as r:
        (ms,) = median_ms(r, (r.render_moments,))
    print(json.dumps({"scene": "demo2", "size": [W, H], "root": root, "spp": root * root, "reps": reps, "uniform_moments_ms": round(ms, 3)}), flush=True)
