"""The host half of context creation (flux_amd/csrc/scene_build.cpp) checked on the CPU: tests/scene_build_selftest.cpp builds the
records, the FAST scene image, the mesh's triangles and trees and the scene-derived RenderParams of four shipped scenes and a
height field, and this test pins the SHA-256 of every buffer.  The digests are the bytes the kernels read: a change to any of
them changes what a context uploads.  The same program asks the launch planner (flux_amd/csrc/launch_plan.cpp) which kernel
instantiation, block, grid and LDS each of those scenes gets over a grid of jobs; the table is pinned too, and so is the
instantiation word of the headline job (demo2, 800 x 600, 16384 spp, depth 5) and of box_room at depths 5 and 3 ("ok flags").
Every one of those plans, and every plan of a grid of synthetic jobs the shipped scenes do not reach ("ok synthetic plans"), must
name a kernel instantiation that render.hip compiles (flux_plan.h kernel_exists): a planner that asks for one that is not there
fails here, not at a launch on a GPU.  The program runs once more as a stand-alone executable under AddressSanitizer and UBSan."""
import hashlib
import os

import pytest

import selftest as st
import switches
from conftest import SCENES

BUFFERS = ("shapes", "mats", "fscene", "tris", "nodes", "nodesq", "arena", "scalars")
SCENE_NAMES = ("demo1", "demo2", "disk_light", "glass", "heightfield")

DIGESTS = {
    "demo1.arena": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "demo1.fscene": "44a7ad117428bdf2d150bb1c08426a4e677d8e046ea209404c26b91d7a01384c",
    "demo1.mats": "bb4a57006db7100f93b01c20997bd96af88fa19e2590a3079cfebe51788f8188",
    "demo1.nodes": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "demo1.nodesq": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "demo1.scalars": "913a85df95c3b455156d048976386062c8ecc26bda14b291e4ac6b65d768d8a4",
    "demo1.shapes": "1f9a67127ec6577b5994cc74e38149a6b5e72795330c7c06f06f1f40e5a2f217",
    "demo1.tris": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "demo2.arena": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "demo2.fscene": "8f53b6c44df12e2b3d77c267a0092f9e8fe31418f75bd913fa22560f3836475d",
    "demo2.mats": "6df6d78ad23cfb337685d9eb030d01079f3f9c32dc95bcce45d92f17b09756ca",
    "demo2.nodes": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "demo2.nodesq": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "demo2.scalars": "22936df35a0fe7b3f986e644337988282a68ce53c7d44e77fe45c36c8d5389af",
    "demo2.shapes": "db278296bd9ce8d1ecc7f739f4f3e3f52c7204369990d7a3c47c74a514251238",
    "demo2.tris": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "disk_light.arena": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "disk_light.fscene": "a94b1a6bc3f70869a304fc6a8fd44982904cfc0c2b04e4a015cbd8c528e2e262",
    "disk_light.mats": "6df6d78ad23cfb337685d9eb030d01079f3f9c32dc95bcce45d92f17b09756ca",
    "disk_light.nodes": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "disk_light.nodesq": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "disk_light.scalars": "9faa7e7c7d0da08ca00bda6973319d82b8673edf7029152f56ed23da6d5663c6",
    "disk_light.shapes": "a5b0e1869bee7d678a6b80fe0308d9a878dc2e21d250f42ce11f686ca915f887",
    "disk_light.tris": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "glass.arena": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "glass.fscene": "a5732247d4dae5aa0fbae2384b218f36070b1be2443630092c6f710858030d1c",
    "glass.mats": "8311ec99579711c08d35d9569898bcb0548e38d89549159929c6d1fd0649c87b",
    "glass.nodes": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "glass.nodesq": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "glass.scalars": "5fd87304288088934ca3decd4cb6811aaa693460e5c75521357c4f3b51e889eb",
    "glass.shapes": "db278296bd9ce8d1ecc7f739f4f3e3f52c7204369990d7a3c47c74a514251238",
    "glass.tris": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "heightfield.arena": "fdad34fc17314c27a22c0c7f68121fd733472e3401f16c59d32eef744139c70a",
    "heightfield.fscene": "44a7ad117428bdf2d150bb1c08426a4e677d8e046ea209404c26b91d7a01384c",
    "heightfield.mats": "1a9eb1d0dc5931b3b7b5afd5b67a3b4d92e6eee3ea48e458214c356c0bf5fe99",
    "heightfield.nodes": "24cc7e9e897e98e350a95285fa00c108837cf3ba510ab9ccac4b30629d527b57",
    "heightfield.nodesq": "2b246b05689b6ce6804f9c17cbf0747633dec19cffd2d6441066ef1f2cc084c6",
    "heightfield.scalars": "cce1abccf3ead8acf421db2cf2fc3ae7eb6c8ae19f46d045e86804c4462c68a3",
    "heightfield.shapes": "1f9a67127ec6577b5994cc74e38149a6b5e72795330c7c06f06f1f40e5a2f217",
    "heightfield.tris": "0e011d18a8dff082ab7e97d085a68aeb8819c396fed86ecb00352d35604e02b0",
}


# plans.txt: 5 scenes x sample roots 4 / 8 / 16 / 128 x 4 kernel variants x FAST / STRICT x 3 traversals x a rows and a sets launch,
# then the same under FLUX_SPLIT_HITQ_CAP=0 (one line each)
PLANS_SHA256 = "12f2966b8918c2997213ead19f3703bc8454ff8affb538bf20b229de6838fa32"
# pass_plans.txt: 5 scenes x sample roots 2 / 3 / 8 / 10 / 16 x FAST / STRICT x 3 traversals x the passes aov, moments, adaptive
# over one list entry and adaptive over npix / 7 + 1 entries: copy, tris, block, blocks and lds (one line each)
PASS_PLANS_SHA256 = "f030afc9ade51a7de2755ff925caa85ca01339619a6d61196532ec8b3c092fef"


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    return st.build(str(tmp_path_factory.mktemp("scene_build") / "scene_build_selftest"), "scene_build_selftest.cpp",
                    csrc=("scene_build.cpp", "bvh.cpp"))


def _run(exe, out_dir, threads=None):
    os.makedirs(out_dir, exist_ok=True)
    stdout = st.run(exe, SCENES, str(out_dir), env=switches.clean_env(FLUX_BUILD_THREADS=threads))
    digests = {}
    for scene in SCENE_NAMES:
        for buf in BUFFERS:
            ext = "txt" if buf == "scalars" else "bin"
            with open(os.path.join(out_dir, f"{scene}.{buf}.{ext}"), "rb") as f:
                digests[f"{scene}.{buf}"] = hashlib.sha256(f.read()).hexdigest()
    return stdout, digests


@pytest.fixture(scope="module")
def default_out(tmp_path_factory):
    return tmp_path_factory.mktemp("default")


@pytest.fixture(scope="module")
def default_run(selftest, default_out):
    return _run(selftest, default_out)


def test_selftest_checks(default_run):
    stdout, _ = default_run
    for name in ("unit normal", "non-unit plane normal", "sphere beyond 1e3", "one emissive invert sphere", "two invert spheres",
                 "group walk", "no f32 filter", "plans", "synthetic plans", "flags") + tuple(f"dump {s}" for s in SCENE_NAMES):
        assert f"ok {name}" in stdout
    assert "all ok" in stdout


def test_selftest_under_asan_and_ubsan(tmp_path):
    """The host build, the planner (compiled into the program) and the walk over its answers with -fsanitize=address,undefined."""
    exe = st.build(str(tmp_path / "scene_build_selftest_san"), "scene_build_selftest.cpp",
                   csrc=("scene_build.cpp", "bvh.cpp", "launch_plan.cpp"), flags=st.SANITIZE)
    assert "all ok" in st.run(exe, SCENES, str(tmp_path), env=st.sanitize_env(), timeout=600)


def test_buffers_are_pinned(default_run):
    _, digests = default_run
    assert digests == DIGESTS


def test_mesh_is_the_same_with_one_thread(selftest, default_run, tmp_path):
    _, digests = _run(selftest, tmp_path, threads=1)
    assert {k: v for k, v in digests.items() if k.startswith("heightfield.")} == \
           {k: v for k, v in default_run[1].items() if k.startswith("heightfield.")}


def _plans(out_dir):
    rows = {}
    with open(os.path.join(out_dir, "plans.txt")) as f:
        for line in f:
            head, _, rest = line.partition(" kernel=")
            rows[head] = dict(kv.split("=") for kv in ("kernel=" + rest).split())
    return rows


def test_pass_plans_are_pinned(default_run, default_out):
    with open(os.path.join(default_out, "pass_plans.txt"), "rb") as f:
        text = f.read()
    assert len(text.splitlines()) == 5 * 5 * 2 * 3 * 4
    assert hashlib.sha256(text).hexdigest() == PASS_PLANS_SHA256


def test_launch_plans_are_pinned(default_run, default_out):
    with open(os.path.join(default_out, "plans.txt"), "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == PLANS_SHA256
    plans = _plans(default_out)
    assert len(plans) == 5 * 4 * 4 * 2 * 3 * 2 * 2

    def plan(scene, math="fast", traversal="bvh", launch="rows", root=128, variant="default"):
        return plans[f"{scene} root={root} variant={variant} math={math} traversal={traversal} launch={launch}"]

    # demo2 at 16384 spp: the split kernel, 4 waves per pixel, the hit queue of 110 slots taken at H = 46, the TYP instantiation
    p = plan("demo2")
    assert (p["kernel"], p["K"], p["hq_cap"], p["hq_th"], p["typ"], p["max32"], p["copy"]) == ("2", "4", "110", "46", "1", "1", "1")
    assert plan("demo2+hitq_cap0")["hq_cap"] == "0"
    # glass: the split kernel with the ray queue, not TYP, in the copy with the dielectric lobe
    p = plan("glass")
    assert (p["kernel"], p["hq_cap"], p["typ"], p["copy"]) == ("2", "0", "0", "2")
    # the height field: the 4-wide tree's kernel, and the binary tree's under FLUX_TRAVERSE_BVH_BINARY
    assert plan("heightfield")["kernel"] == "4"
    assert plan("heightfield", traversal="binary")["kernel"] == "3"
    # demo2 in STRICT: the refill kernel in the STRICT copy
    p = plan("demo2", math="strict")
    assert (p["kernel"], p["copy"]) == ("1", "0")
    # no plan asks the copy with the dielectric lobe for an instantiation it does not compile (TYP, the hit queue)
    assert all(r["typ"] == "0" and r["hq_cap"] == "0" for r in plans.values() if r["copy"] == "2")
