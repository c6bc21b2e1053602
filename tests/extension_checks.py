"""What the suites of the extensions (Disk, Dielectric, Box: tests/test_gpu_*.py and tests/test_*_scene.py) share with each other
and with the headline, parity and host tests: one render with statistics, a frame put together from set shares, row tiles or
loopback ranks, a shipped YAML scene shrunk as text, the command-line tools writing a frame, and the output of a
tests/*_host_selftest.cpp.  Plain functions: each test states its own scenes, worlds, modes and assertions."""
import os
import re
import subprocess
import time

import numpy as np

from conftest import ROOT

HOST = os.path.join(ROOT, "flux_amd", "host")


def math_mode(flux, name):
    return {"fast": flux.MATH_FAST, "strict": flux.MATH_STRICT}[name]


def render(flux, sd, n, math_mode, kernel=None, traversal=None, seed=1, depth=5):
    """One frame at n x n samples: (image, path statistics, launch plan)."""
    with flux.Renderer(sd, flux.JobConfiguration(n, depth, 50), seed=seed) as r:
        r.set_math(math_mode)
        if kernel is not None:
            r.set_kernel(kernel)
        if traversal is not None:
            r.set_traversal(traversal)
        r.enable_stats(True)
        r.stats(reset=True)
        img = r.render_frame()
        return img, r.stats(), r.launch_plan()


# ---- a box as triangles -------------------------------------------------------------------------------------------------

def box_as_mesh(flux, b):
    """The box `b` as a 12-triangle mesh of the same material, wound outwards (inwards for an inverted box)."""
    from flux_amd.scene import MeshData
    c0, c1 = np.array(b.corner0), np.array(b.corner1)
    v = np.array([[x, y, z] for x in (c0[0], c1[0]) for y in (c0[1], c1[1]) for z in (c0[2], c1[2])])
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tris = np.array([t for a, bb, c, dd in quads for t in ((a, bb, c), (a, c, dd))], dtype=np.uint32)
    ctr = v[tris].mean(axis=1) - 0.5 * (c0 + c1)
    nrm = np.cross(v[tris[:, 1]] - v[tris[:, 0]], v[tris[:, 2]] - v[tris[:, 0]])
    flip = (np.einsum("ij,ij->i", nrm, ctr) < 0) != bool(b.invert)  # outward winding; inwards for an inverted box
    tris[flip] = tris[flip][:, [0, 2, 1]]
    return MeshData(v, tris, b.material)


# ---- a frame from shares ------------------------------------------------------------------------------------------------

def set_sharded_frame(flux, r, world, check_plan=False):
    """The frame (a CPU tensor) assembled from the `world` per-rank set shares, rendered one after the other on this GPU.
    check_plan: every share is launched with as many waves per pixel as the whole frame."""
    import torch
    from flux_amd.dist import SetSharder, hip_render_sets_fn
    dev = torch.device("cuda", 0)
    rowperm = torch.from_numpy(r.row_perm_table())
    fn = hip_render_sets_fn(r)
    shards = []
    for rank in range(world):
        sh = SetSharder(r.height, r.width, rank, world, dev, rowperm)
        if check_plan:
            assert r.launch_plan(num_sets=sh.count)["waves_per_pixel"] == r.launch_plan()["waves_per_pixel"]
        sh.render(fn)
        torch.cuda.synchronize()
        if sh.local is not sh.render_buf:
            sh.local[:, : sh.count] = sh.render_buf
        shards.append(sh)
    s0 = shards[0]
    if world == 1:
        return s0.assemble().cpu()
    gathered = torch.stack([s.local for s in shards])  # what all_gather_into_tensor produces
    return gathered[s0._g, s0._r, s0._m].cpu()


def loopback_frames(flux, sd, cfg, seed, worlds, modes):
    """(G, mode, frame) of a MultiRenderer whose G ranks all sit on device 0, for every G of `worlds` and shard mode of `modes`."""
    for G in worlds:
        for mode in modes:
            with flux.MultiRenderer(sd, cfg, seed=seed, devices=[0] * G, shard=mode | flux._lib.SHARD_LOOPBACK) as m:
                yield G, mode, m.render_frame()


def row_tiles(r, step):
    """The frame as row tiles of `step` rows (the last one shorter), stacked."""
    return np.concatenate([r.render_rows(a, min(a + step, r.height) - 1) for a in range(0, r.height, step)], axis=0)


# ---- the command-line tools ---------------------------------------------------------------------------------------------

def small_yaml(path, tmp_path, w, h, edits=()):
    """The shipped 800 x 600 scene `path`, shrunk as text to w x h with the same field of view (and with the (old, new) pairs of
    `edits` applied), written under tmp_path: the new path.  Every replacement must match exactly once."""
    text = open(path).read()
    for old, new in (("image_width: 800", f"image_width: {w}"), ("image_height: 600", f"image_height: {h}"),
                     ("pixel_size: 0.5", f"pixel_size: {0.5 * 800 / w!r}"), *edits):
        assert text.count(old) == 1, (path, old, text.count(old))
        text = text.replace(old, new)
    out = tmp_path / os.path.basename(path)
    out.write_text(text)
    return str(out)


def host_bins():
    """The paths of the built `flux` and `flux_node`."""
    from flux_amd import build
    build.build_host()
    return os.path.join(HOST, "flux"), os.path.join(HOST, "flux_node")


def _ppm(scene, outdir):
    return open(os.path.join(outdir, os.path.splitext(os.path.basename(scene))[0] + ".ppm"), "rb").read()


def cli_frame(flux_bin, scene, args, outdir):
    """`flux <scene> <args> --gpus 1 --outdir <outdir>`: the bytes of the PPM it wrote."""
    os.makedirs(outdir)
    r = subprocess.run([flux_bin, scene, *args, "--gpus", "1", "--outdir", str(outdir)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return _ppm(scene, outdir)


def node_frame(flux_bin, node_bin, scene, args, outdir, tmp_path, stdout_has=()):
    """`flux <scene> <args> -L -n <a flux_node --once on this machine>`: the bytes of the PPM it wrote.  The node takes the `--seed` of
    `args`, logs to tmp_path/node.log and must exit with status 0; `stdout_has` are strings that the client must print."""
    os.makedirs(outdir)
    log_path = tmp_path / "node.log"
    log = open(log_path, "w")
    node = subprocess.Popen([node_bin, "-h", "127.0.0.1", "-p", "0", "-t", "4", "--seed", args[args.index("--seed") + 1], "--once"],
                            stdout=log, stderr=subprocess.STDOUT, text=True)
    try:
        port = None
        for _ in range(600):
            m = re.search(r"Listening on port (\d+)", open(log_path).read())
            if m:
                port = m.group(1)
                break
            assert node.poll() is None, open(log_path).read()
            time.sleep(0.05)
        assert port, "flux_node did not come up"
        r = subprocess.run([flux_bin, scene, *args, "-L", "-n", f"127.0.0.1:{port}", "--outdir", str(outdir)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr + r.stdout
        for s in stdout_has:
            assert s in r.stdout, r.stdout
        assert node.wait(timeout=30) == 0
    finally:
        if node.poll() is None:
            node.kill()
        log.close()
    return _ppm(scene, outdir)


# ---- what a tests/<name>_host_selftest.cpp prints (tests/selftest.py builds and runs it) ---------------------------------------------

def cpp_shapes(stdout):
    """The selftest's `shape <i> <fields>` lines as {i: fields}, typed as shape_fields gives them."""
    cpp = {}
    for line in stdout.splitlines():
        if line.startswith("shape "):
            tok = line.split()
            cpp[int(tok[1])] = [int(tok[2]), int(tok[3])] + [float(x) for x in tok[4:11]] + [int(tok[11])] + [float(x) for x in tok[12:]]
    return cpp


def shape_fields(s):
    """The fields of a flux_shape of flux_amd.scene.SceneDesc, in the order the selftests print them."""
    m = s.material
    return [s.kind, s.invert, *s.p, *s.n, s.radius, m.kind, *m.color, *m.ambient, m.k, m.exponent]
