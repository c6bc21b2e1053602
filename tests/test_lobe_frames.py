"""The split kernel's lobe-frame table on the CPU (scene_build.cpp lobe_frame_table): tests/lobe_frame_selftest.cpp holds which hit
records get an entry -- demo2's one plane and none of its spheres, a disk scene's plane and disk, all six face records of every box
of a box scene -- against the records' shape kinds and the YAML's shapes, checks the table's byte size (48 B a record) and that
FLUX_LOBE_FRAMES=0 yields no table.  The program is run once more as a stand-alone executable under AddressSanitizer and UBSan.
(The entries themselves are the device's work: tests/test_gpu_lobe_frames.py.)"""
import os
import subprocess

import pytest

from conftest import ROOT, SCENES

CHECKS = ("demo2", "disk", "box", "switch")


def _build_selftest(exe, extra=()):
    """Host-only clang and -ffp-contract=off, as tests/test_scene_build.py."""
    from flux_amd import build
    build.build_hip()
    host = os.path.join(ROOT, "flux_amd", "host")
    csrc = os.path.join(ROOT, "flux_amd", "csrc")
    subprocess.run(["/opt/rocm/llvm/bin/clang++", "-O2", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-pthread", "-Wall", *extra, "-o", exe, os.path.join(ROOT, "tests", "lobe_frame_selftest.cpp"),
                    os.path.join(csrc, "scene_build.cpp"), os.path.join(csrc, "bvh.cpp"), os.path.join(csrc, "launch_plan.cpp")] +
                   [os.path.join(host, s) for s in build.HOST_SOURCES] +
                   ["-L" + os.path.join(ROOT, "flux_amd"), "-lflux_hip", "-Wl,-rpath," + os.path.join(ROOT, "flux_amd"),
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def _env(**more):
    env = {k: v for k, v in os.environ.items() if k != "FLUX_LOBE_FRAMES"}
    env.update(more)
    return env


@pytest.fixture(scope="module")
def selftest_out(tmp_path_factory):
    exe = _build_selftest(str(tmp_path_factory.mktemp("lobe") / "lobe_frame_selftest"))
    out = subprocess.run([exe, SCENES], capture_output=True, text=True, env=_env(), timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return out.stdout


@pytest.mark.parametrize("name", CHECKS)
def test_which_records_get_an_entry(selftest_out, name):
    assert f"ok {name}" in selftest_out
    assert "all ok" in selftest_out


def test_selftest_under_asan_and_ubsan(tmp_path):
    """The host function, the scene build and the loaders compiled into a stand-alone executable with -fsanitize=address,undefined."""
    exe = _build_selftest(str(tmp_path / "lobe_frame_selftest_san"),
                          ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"))
    out = subprocess.run([exe, SCENES], capture_output=True, text=True, timeout=300,
                         env=_env(ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert out.returncode == 0 and "all ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
