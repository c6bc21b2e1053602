"""What interpolated normals buy the measured-variance denoiser, on the CPU from the numpy specs alone:
scenes/smooth_sphere.yml's first GlossyReflective sphere over the scene's floor and lights at 64 x 48, once with its vertex normals
and once without, the noisy frame, its moments and its first-hit feature buffers at sample root 2, seed 7, from
tests/smooth_path_spec.py, denoised by tests/denoise_moments_spec.py and held against the same reference at sample root 40, seed 11
(section 5f's and 5g's settings).  MSE over the frame and over the pixels whose every root-2 sample hits the sphere first.
Development aid: the figures of section 5j.  The root-40 references take a quarter of an hour of one core per row block.
usage: smooth_quality.py [--ref-root 40] [--procs 8] [--zoom 1.0]"""
import copy
import json
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, DEPTH = 64, 48, 5


def scene(smooth, zoom):
    import flux_amd
    from conftest import small_scene
    from flux_amd.scene import MeshData
    sd = small_scene(flux_amd.load_scene(os.path.join(ROOT, "scenes", "smooth_sphere.yml")), W, H)
    meshes = [s for s in sd.shapes if isinstance(s, MeshData)]
    ball = copy.deepcopy(meshes[0])
    if not smooth:
        ball.normals = None
    sd.shapes = [s for s in sd.shapes if not isinstance(s, MeshData)] + [ball]
    sd.camera_data.zoom_factor *= zoom
    c = np.asarray(ball.vertices).mean(axis=0)
    sd.camera_settings.look_at = tuple(float(x) for x in c)
    return sd


def rows_mean(args):
    """[len(rows), W, 3]: the sample mean (before max_to_one) of the rows at the reference's root"""
    smooth, zoom, root, seed, rows = args
    import smooth_path_spec
    spec = smooth_path_spec.SmoothPathSpec(scene(smooth, zoom), root, DEPTH, seed)
    N = root * root
    out = np.zeros((len(rows), W, 3))
    for k, row in enumerate(rows):
        perm = spec._oracle.row_perm(row)
        o, d, sets = np.empty((W, N, 3)), np.empty((W, N, 3)), np.empty(W, dtype=int)
        for col in range(W):
            sets[col] = int(perm[col]) % W
            for i in range(N):
                o[col, i], d[col, i] = spec._oracle.primary_ray(row, col, sets[col], i)
        rad = spec._trace(o.reshape(-1, 3), d.reshape(-1, 3), np.repeat(sets, N), np.tile(np.arange(N), W))[0].reshape(W, N, 3)
        color = np.zeros((W, 3))
        for i in range(N):
            color = color + rad[:, i]
        out[k] = color * (1.0 / float(N))
    spec.close()
    return out


def main():
    args = sys.argv[1:]
    opt = lambda name, default: type(default)(args[args.index(name) + 1]) if name in args else default  # noqa: E731
    ref_root, procs, zoom = opt("--ref-root", 40), opt("--procs", 8), opt("--zoom", 1.0)
    import denoise_moments_spec as dms
    import denoise_spec
    import moments_spec as ms
    import path_spec
    import smooth_path_spec
    from oracle import oracle as oracle_mod
    result = {"width": W, "height": H, "ref_root": ref_root, "zoom": zoom}
    with multiprocessing.Pool(procs) as pool:
        for smooth in (False, True):
            blocks = pool.map(rows_mean, [(smooth, zoom, ref_root, 11, list(range(a, H, procs * 2))) for a in range(procs * 2)])
            mean = np.zeros((H, W, 3))
            for a, b in enumerate(blocks):
                mean[a::procs * 2] = b
            ref = np.array([[oracle_mod.max_to_one(mean[r, c]) for c in range(W)] for r in range(H)])
            spec = smooth_path_spec.SmoothPathSpec(scene(smooth, zoom), 2, DEPTH, 7)
            noisy = spec.frame()
            mom = ms.from_samples(spec.sample_radiance)
            aov = path_spec.aov_buffers(spec)
            ball = (spec.first_hits()[0] == len(spec.sd.shapes) - 1).all(axis=2)
            spec.close()
            den = dms.denoise_moments(mom, aov)
            key = "smooth" if smooth else "flat"
            result[key] = {"sphere_pixels": int(ball.sum()),
                           "mse_noisy": denoise_spec.mse(noisy, ref), "mse_denoised": denoise_spec.mse(den, ref),
                           "mse_noisy_sphere": float(((noisy - ref) ** 2)[ball].mean()), "mse_denoised_sphere": float(((den - ref) ** 2)[ball].mean())}
            result[key]["ratio"] = result[key]["mse_denoised"] / result[key]["mse_noisy"]
            result[key]["ratio_sphere"] = result[key]["mse_denoised_sphere"] / result[key]["mse_noisy_sphere"]
            print(json.dumps({key: result[key]}), flush=True)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
