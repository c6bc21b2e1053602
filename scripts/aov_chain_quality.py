"""Whether chain guides (flux_render_aov_chain_rows) improve the measured-variance denoiser's frame: for the
shipped scenes with mirrors or glass at 64 x 48, seed 7, depth 5, the MSE of denoise_moments with first-hit guides and with chain
guides at sample roots 2 and 4 against the same Renderer at 4096 spp under seed 11, over the whole frame and over the "delta
pixels": those whose chain depth differs from their first-hit depth, i.e. with a sample that a mirror or glass sent on.  Development aid: the figures of section 5i's table.
usage: aov_chain_quality.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import flux_amd  # noqa: E402
from conftest import small_scene  # noqa: E402

W, H = 64, 48


def mse(x, ref, mask=None):
    d = (np.asarray(x) - ref) ** 2
    return float(d.mean() if mask is None else d[mask].mean())


for name in ("glass", "mirror_glass"):
    sd = small_scene(flux_amd.load_scene(os.path.join(ROOT, "scenes", name + ".yml")), W, H)
    with flux_amd.Renderer(sd, flux_amd.JobConfiguration(64, 5, 50), seed=11) as r:
        ref = r.render_frame()
    for root in (2, 4):
        with flux_amd.Renderer(sd, flux_amd.JobConfiguration(root, 5, 50), seed=7) as r:
            mom, first, chain = r.render_moments(), r.render_aov(), r.render_aov_chain()
            noisy = mom[..., 0:3]
            a, b = flux_amd.denoise_moments(mom, first), flux_amd.denoise_moments(mom, chain)
            sa, sb = flux_amd.denoise(noisy, first), flux_amd.denoise(noisy, chain)
        # the pixels that see a mirror or glass first: where following the chain moves the depth
        with np.errstate(invalid="ignore"):
            delta = np.abs(chain[..., 6] - first[..., 6]) > 1e-9 * np.maximum(1.0, np.abs(first[..., 6]))
        out = {"scene": name, "spp": root * root, "delta_pixels": int(delta.sum()), "pixels": W * H}
        for label, mask in (("frame", None), ("delta", delta)):
            base = mse(noisy, ref, mask)
            out[label] = {"mse_noisy": base, "measured_first": round(mse(a, ref, mask) / base, 4), "measured_chain": round(mse(b, ref, mask) / base, 4),
                          "chain_over_first_measured": round(mse(b, ref, mask) / mse(a, ref, mask), 4),
                          "spatial_first": round(mse(sa, ref, mask) / base, 4), "spatial_chain": round(mse(sb, ref, mask) / base, 4),
                          "chain_over_first_spatial": round(mse(sb, ref, mask) / mse(sa, ref, mask), 4)}
        print(json.dumps(out), flush=True)
