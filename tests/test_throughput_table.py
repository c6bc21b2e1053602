"""The split kernel's throughput product table (flux_plan.h tput_index, scene_build.cpp build_tput_table) and the hit queue's slot on
the CPU: tests/throughput_table_selftest.cpp holds every table entry of demo2 and of a 16-record scene against the product the
kernel's loop forms (bit patterns), checks the index of (n, ml), the slot's field offsets and which jobs get a table, and prints the
launch planner's answer for the shipped scenes, whose every reported field is pinned here.  The program is run once more as a
stand-alone executable under AddressSanitizer and UBSan."""
import os
import subprocess

import pytest

from conftest import ROOT, SCENES

# scene, sample root -> kernel, block, blocks, lds, waves per pixel, hq_cap, hq_th, hq_bits, typ, max32 (what the planner answered
# before the table existed: the table changes no plan)
PLANS = {
    ("demo1", 16): (2, 64, 480000, 7536, 1, 100, 36, 3, 1, 1), ("demo1", 128): (2, 256, 480000, 31744, 4, 114, 50, 3, 1, 1),
    ("demo2", 16): (2, 64, 480000, 6752, 1, 0, 0, 0, 1, 1), ("demo2", 128): (2, 256, 480000, 31552, 4, 110, 46, 4, 1, 1),
    ("disk_light", 16): (2, 64, 480000, 6720, 1, 0, 0, 0, 0, 1), ("disk_light", 128): (2, 256, 480000, 31520, 4, 110, 46, 4, 0, 1),
    ("box_room", 16): (2, 64, 480000, 7072, 1, 0, 0, 0, 0, 1), ("box_room", 128): (2, 256, 480000, 31872, 4, 110, 46, 5, 0, 1),
    ("glass", 16): (2, 64, 480000, 6752, 1, 0, 0, 0, 0, 1), ("glass", 128): (2, 256, 480000, 22112, 4, 0, 0, 0, 0, 1),
}
CHECKS = ("slot", "index", "table", "plans", "which jobs")


def _build_selftest(exe, extra=()):
    """Host-only clang and -ffp-contract=off, as tests/test_scene_build.py: the products are plain IEEE multiplications."""
    from flux_amd import build
    build.build_hip()
    host = os.path.join(ROOT, "flux_amd", "host")
    csrc = os.path.join(ROOT, "flux_amd", "csrc")
    subprocess.run(["/opt/rocm/llvm/bin/clang++", "-O2", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-pthread", "-Wall", *extra, "-o", exe, os.path.join(ROOT, "tests", "throughput_table_selftest.cpp"),
                    os.path.join(csrc, "scene_build.cpp"), os.path.join(csrc, "bvh.cpp"), os.path.join(csrc, "launch_plan.cpp")] +
                   [os.path.join(host, s) for s in build.HOST_SOURCES] +
                   ["-L" + os.path.join(ROOT, "flux_amd"), "-lflux_hip", "-Wl,-rpath," + os.path.join(ROOT, "flux_amd"),
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def _env(**more):
    env = {k: v for k, v in os.environ.items() if k not in ("FLUX_SPLIT_HITQ_CAP", "FLUX_SPLIT_HITQ_TAKE_AT")}
    env.update(more)
    return env


@pytest.fixture(scope="module")
def selftest_out(tmp_path_factory):
    exe = _build_selftest(str(tmp_path_factory.mktemp("tput") / "throughput_table_selftest"))
    out = subprocess.run([exe, SCENES], capture_output=True, text=True, env=_env(), timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return out.stdout


def test_table_index_and_slot(selftest_out):
    for name in CHECKS:
        assert f"ok {name}" in selftest_out
    assert "all ok" in selftest_out


def test_shipped_scenes_keep_their_plans(selftest_out):
    got = {}
    for line in selftest_out.splitlines():
        if line.startswith("plan "):
            w = line.split()
            f = dict(kv.split("=") for kv in w[2:])
            got[(w[1], int(f["root"]))] = tuple(int(f[k]) for k in ("kernel", "block", "blocks", "lds", "K", "hq_cap", "hq_th", "hq_bits",
                                                                    "typ", "max32"))
    assert got == PLANS


def test_selftest_under_asan_and_ubsan(tmp_path):
    """The table's builder, the planner and the loaders compiled into a stand-alone executable with -fsanitize=address,undefined."""
    exe = _build_selftest(str(tmp_path / "throughput_table_selftest_san"),
                          ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"))
    out = subprocess.run([exe, SCENES], capture_output=True, text=True, timeout=300,
                         env=_env(ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert out.returncode == 0 and "all ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
