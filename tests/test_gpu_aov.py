"""The first-hit feature buffers on the GPU (flux_render_aov_rows*) against their specification in Python
(tests/aov_spec.py): parity in both arithmetics, meshes in the three traversals, the extension shapes, the tie to the production
kernels' rays, the calls, the absence of side effects, and the command-line tool.

All scenes are 16 x 12 at seed 7.  Tolerance: |Δ| <= 1e-9 on channels 0-5 and 7, |Δ| <= 1e-9 max(1, depth) on depth, every pixel --
the whole-frame agreement of the kernels with the restatement is 5.2e-13, t is below ~110, so differences near 1e-11 are expected;
1e-9 leaves two decades and is four decades below one flipped sample at 100 spp (1e-2).  No pixel is excluded: every sample's
first-hit decision survives a 1e-11 relative perturbation of origin and direction."""
import os

import numpy as np
import pytest

import aov_spec
from conftest import SCENES, small_scene
from extension_checks import cli_frame, host_bins, math_mode, small_yaml

pytestmark = pytest.mark.gpu

MATHS = ("fast", "strict")
# the restatement's counts (aov_spec.reference on the CPU): scene, sample_root -> misses, partly covered pixels
OPEN_FACTS = {1: (19, 0), 3: (181, 13), 8: (1245, 17), 10: (1948, 21)}


def gpu_aov(flux, sd, root, math, traversal=None, seed=aov_spec.SEED):
    with flux.Renderer(sd, flux.JobConfiguration(root, 5, 50), seed=seed) as r:
        r.set_math(math_mode(flux, math))
        if traversal is not None:
            r.set_traversal(traversal)
        return r.render_aov()


_refs = {}


def spec(flux, oracle_mod, name, root):
    """The specification's buffers and counts, computed once per (scene, sample_root) and shared, read-only."""
    if (name, root) not in _refs:
        if name == "open":
            sd = aov_spec.open_scene(flux)
        elif name == "open_mesh":
            sd = aov_spec.open_mesh_scene(flux)
        else:
            sd = small_scene(flux.load_scene(os.path.join(SCENES, name + ".yml")), aov_spec.W, aov_spec.H)
        aov, facts = aov_spec.reference(oracle_mod, sd, root)
        aov.setflags(write=False)
        _refs[(name, root)] = (sd, aov, facts)
    return _refs[(name, root)]


# ---- 1. parity with the spec --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("name,root", [("open", 1), ("open", 3), ("open", 8), ("open", 10), ("demo1", 8), ("demo2", 8)])
def test_parity_with_the_spec(flux, oracle_mod, name, root, math):
    """Lane groups with an idle tail (root 3: 7 pixels of 9 lanes a wave), lane groups of one lane (root 1), exactly one chunk
    (root 8), a partial second chunk (root 10); demo1 and demo2 with their inverted environment sphere."""
    sd, want, facts = spec(flux, oracle_mod, name, root)
    got = gpu_aov(flux, sd, root, math)
    aov_spec.assert_close(got, want, f"{name} root {root} {math}")
    cov = got[..., aov_spec.COVERAGE]
    N = root * root
    if name == "open":
        misses, partly = OPEN_FACTS[root]
        assert (facts["misses"], facts["partly_covered"], facts["samples"]) == (misses, partly, aov_spec.W * aov_spec.H * N)
        assert np.count_nonzero((cov > 0) & (cov < 1)) == partly
        assert round(float((1.0 - cov).sum() * N)) == misses
    else:
        assert facts["misses"] == 0 and np.all(cov == 1.0)  # a closed scene: coverage is exactly 1


# ---- 2. meshes ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("math", MATHS)
def test_meshes_in_the_three_traversals(flux, oracle_mod, math):
    sd, want, facts = spec(flux, oracle_mod, "open_mesh", 8)
    assert (facts["misses"], facts["samples"], facts["partly_covered"]) == (838, 12288, 17)
    L = flux._lib
    frames = {}
    for name, mode in (("bvh", L.TRAVERSE_BVH), ("brute", L.TRAVERSE_BRUTE), ("binary", L.TRAVERSE_BVH_BINARY)):
        frames[name] = gpu_aov(flux, sd, 8, math, traversal=mode)
        aov_spec.assert_close(frames[name], want, f"open_mesh root 8 {math} {name}")
    assert np.array_equal(frames["bvh"], frames["brute"]) and np.array_equal(frames["bvh"], frames["binary"])
    cov = frames["bvh"][..., aov_spec.COVERAGE]
    assert np.count_nonzero((cov > 0) & (cov < 1)) == 17
    # the quad's Matte albedo is seen somewhere on its own: a pixel all of whose samples hit it
    assert np.any(np.all(np.abs(frames["bvh"][..., aov_spec.ALBEDO] - 0.8 * np.array([0.2, 0.7, 0.3])) < 1e-12, axis=2))


# ---- 3. extension shapes --------------------------------------------------------------------------------------------------------

# disk_light as shipped looks down on the floor from below its downward-facing disk: none of its 12 288 samples meets the disk
# (counted on the CPU from the restatement's rays), so the frame is compared as it is and the disk is asserted as a first hit in a
# second case, the same scene seen from (0, 0.5, -9) towards the disk's centre (1 698 samples on 40 pixels meet its plane within
# its radius).
EXTENSION_CASES = [("box_room", "BoxData", None), ("disk_light", None, None), ("disk_light", "DiskData", ((0.0, 0.5, -9.0), (-9.0, 7.0, 8.0))),
                   ("glass", "DielectricData", None)]


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("name,wanted,camera", EXTENSION_CASES, ids=["box_room", "disk_light", "disk_light_seen", "glass"])
def test_extension_shapes(flux, oracle_mod, name, wanted, camera, math):
    """Disk, Box and Dielectric, which the restatement rejects: its rays, the first hit and t of Renderer.debug_shade, the normal
    by the shape's own rule -- the first hit is the GPU's own here.  The reference that owes the GPU nothing is
    tests/path_spec.py's first_hits(): tests/test_gpu_ext_fuzz.py holds render_aov() against it on its random scenes."""
    sd = small_scene(flux.load_scene(os.path.join(SCENES, name + ".yml")), aov_spec.W, aov_spec.H)
    if camera is not None:
        sd.camera_settings = flux.CameraSettings(camera[0], camera[1], (0.0, 1.0, 0.0))
    want, _, hit = aov_spec.reference_debug_shade(flux, oracle_mod, sd, 8, math_mode(flux, math))
    seen = {type(sd.shapes[k]).__name__ for k in np.unique(hit) if k >= 0}
    seen |= {type(sd.shapes[k].material).__name__ for k in np.unique(hit) if k >= 0}
    if wanted is not None:
        assert wanted in seen, (wanted, sorted(seen))  # the scene's extension is the first hit of at least one sample
    else:
        assert "DiskData" not in seen
    got = gpu_aov(flux, sd, 8, math)
    aov_spec.assert_close(got, want, f"{name}{'' if camera is None else ' (disk in view)'} root 8 {math}")


# ---- 4. the same rays as the render ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("root", [3, 16])
def test_albedo_of_an_emissive_scene_is_the_depth_one_render(flux, root):
    """Every shape Emissive with power * colour <= 1 over a background <= 1: at max_trace_depth 1 a sample's radiance is its
    albedo and max_to_one does nothing, so the frame of each production kernel is the albedo buffer -- same sets, same
    permutation, same primary rays."""
    sd = aov_spec.open_emissive_scene(flux)
    with flux.Renderer(sd, flux.JobConfiguration(root, 1, 50), seed=aov_spec.SEED) as r:
        aov = r.render_aov()
        assert aov[..., aov_spec.ALBEDO].max() <= 1.0
        for kernel in (flux.KERNEL_STATIC, flux.KERNEL_REFILL, flux.KERNEL_SPLIT):
            r.set_kernel(kernel)
            frame = r.render_frame()
            err = float(np.max(np.abs(frame - aov[..., aov_spec.ALBEDO])))
            print(f"aov emissive root {root} kernel {kernel} (plan {r.launch_plan()['kernel']}): max |render - albedo| = {err:.2e}")
            assert err <= 1e-12, (kernel, err)
    cov = aov[..., aov_spec.COVERAGE]
    assert ((cov > 0) & (cov < 1)).any() and (cov == 0).any()


# ---- 5. calls ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("root", [3, 8])
def test_row_tiles_strided_rows_and_refusals(flux, root):
    import torch
    sd = aov_spec.open_scene(flux)
    L = flux._lib
    with flux.Renderer(sd, flux.JobConfiguration(root, 5, 50), seed=aov_spec.SEED) as r:
        frame = r.render_aov()
        assert frame.shape == (aov_spec.H, aov_spec.W, 8)
        tiles = np.concatenate([r.render_aov(a, min(a + 5, r.height) - 1) for a in range(0, r.height, 5)], axis=0)
        assert np.array_equal(tiles, frame)
        assert np.array_equal(r.render_aov(), frame)  # run to run
        rows = list(range(1, aov_spec.H, 2))
        buf = torch.full((len(rows), aov_spec.W, 8), -7.0, dtype=torch.float64, device="cuda:0")
        r.render_aov_device(1, 2, len(rows), buf.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy(), frame[rows])
        assert r.last_kernel_ms() > 0.0  # the launch sits between the context's two events
        buf.fill_(-7.0)
        r.render_aov_device(0, 1, 0, buf.data_ptr())  # num_rows = 0: a no-op
        r.render_aov_device(0, 1, 0, 0)
        torch.cuda.synchronize()
        assert bool((buf == -7.0).all())
        for bad in (lambda: r.render_aov(0, aov_spec.H), lambda: r.render_aov_device(aov_spec.H, 1, 1, buf.data_ptr()),
                    lambda: r.render_aov_device(aov_spec.H - 2, 2, 2, buf.data_ptr()), lambda: r.render_aov_device(0, 0, 1, buf.data_ptr()),
                    lambda: r.render_aov_device(0, 1, 1, 0)):
            with pytest.raises(flux.FluxError) as e:
                bad()
            assert e.value.code == L.E_INVALID
    with flux.Renderer(sd, flux.JobConfiguration(root, 5, 50), seed=aov_spec.SEED, set_share=(1, 2)) as part:
        with pytest.raises(flux.FluxError, match="sample sets") as e:
            part.render_aov()
        assert e.value.code == L.E_INVALID


# ---- 6. no side effects -----------------------------------------------------------------------------------------------------------

def test_no_side_effects(flux, demo2):
    sd = small_scene(demo2, aov_spec.W, aov_spec.H)
    with flux.Renderer(sd, flux.JobConfiguration(8, 5, 50), seed=aov_spec.SEED) as r:
        r.enable_stats(True)
        r.stats(reset=True)
        plan = r.launch_plan()
        before = r.render_frame()
        stats = r.stats()
        assert stats["samples"] == aov_spec.W * aov_spec.H * 64
        aov = r.render_aov()
        assert r.stats() == stats        # the kernel keeps no statistics
        assert r.launch_plan() == plan
        r.stats(reset=True)
        after = r.render_frame()         # the host call's own buffer: the render's scratch framebuffer is untouched
        assert np.array_equal(before, after) and r.stats() == stats
        assert np.array_equal(r.render_aov(), aov)


# ---- 7. the command-line tool -------------------------------------------------------------------------------------------------------

def test_cli_writes_the_four_buffers(flux, tmp_path):
    flux_bin, _ = host_bins()
    scene = small_yaml(os.path.join(SCENES, "demo2.yml"), tmp_path, aov_spec.W, aov_spec.H)
    out = tmp_path / "out"
    frame_ppm = cli_frame(flux_bin, scene, ["-r", "8", "--seed", "5", "--aov"], out)
    sd = flux.load_scene(scene)
    with flux.Renderer(sd, flux.JobConfiguration(8, 5, 50), seed=5) as r:
        aov = r.render_aov()
        flux.write_ppm(str(tmp_path / "frame.ppm"), r.render_frame())
    assert frame_ppm == open(tmp_path / "frame.ppm", "rb").read()
    assert sorted(os.listdir(out)) == sorted([sd.scene_name + ".ppm"] + [f"{sd.scene_name}.{k}.ppm" for k in ("albedo", "normal", "depth", "coverage")])
    for kind in ("albedo", "normal", "depth", "coverage"):
        want = tmp_path / f"want.{kind}.ppm"
        flux.write_ppm(str(want), aov_spec.aov_image(aov, kind))
        assert open(out / f"{sd.scene_name}.{kind}.ppm", "rb").read() == open(want, "rb").read(), kind


def test_cli_refuses_aov_without_a_local_gpu(tmp_path):
    import subprocess
    flux_bin, _ = host_bins()
    scene = small_yaml(os.path.join(SCENES, "demo2.yml"), tmp_path, aov_spec.W, aov_spec.H)
    r = subprocess.run([flux_bin, scene, "-r", "8", "--aov", "--gpus", "0", "--outdir", str(tmp_path / "none")],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--aov" in r.stderr and "local GPU" in r.stderr
    assert not os.path.exists(tmp_path / "none")
