"""When the split kernel's depth cut is admitted, on the CPU (launch_plan.cpp split_cut_depth, scene_build.cpp tput_products_finite):
tests/depth_cut_selftest.cpp holds the context's finiteness check against tables that are finite, tables with an infinite or a NaN
entry, and tables whose entries are finite while the bounce at the depth limit overflows; and the planner's answer for jobs with
and without the table, with the hit queue and with the ray queue, at depth 1, and under FLUX_SPLIT_DEPTH_CUT.  The program is run
once more as a stand-alone executable under AddressSanitizer and UBSan.  GPU side: tests/test_gpu_depth_cut.py."""
import os
import subprocess

import pytest

from conftest import ROOT, SCENES

CHECKS = ("finite tables", "tables that are not finite", "plan")


def _build_selftest(exe, extra=()):
    """Host-only clang and -ffp-contract=off, as tests/test_throughput_table.py: the products are plain IEEE multiplications."""
    from flux_amd import build
    build.build_hip()
    host = os.path.join(ROOT, "flux_amd", "host")
    csrc = os.path.join(ROOT, "flux_amd", "csrc")
    subprocess.run(["/opt/rocm/llvm/bin/clang++", "-O2", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-pthread", "-Wall", *extra, "-o", exe, os.path.join(ROOT, "tests", "depth_cut_selftest.cpp"),
                    os.path.join(csrc, "scene_build.cpp"), os.path.join(csrc, "bvh.cpp"), os.path.join(csrc, "launch_plan.cpp")] +
                   [os.path.join(host, s) for s in build.HOST_SOURCES] +
                   ["-L" + os.path.join(ROOT, "flux_amd"), "-lflux_hip", "-Wl,-rpath," + os.path.join(ROOT, "flux_amd"),
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def _env(**more):
    env = {k: v for k, v in os.environ.items() if k not in ("FLUX_SPLIT_HITQ_CAP", "FLUX_SPLIT_HITQ_TAKE_AT", "FLUX_SPLIT_DEPTH_CUT")}
    env.update(more)
    return env


def test_admission(tmp_path):
    exe = _build_selftest(str(tmp_path / "depth_cut_selftest"))
    out = subprocess.run([exe, SCENES], capture_output=True, text=True, env=_env(), timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    for name in CHECKS:
        assert f"ok {name}" in out.stdout
    assert "all ok" in out.stdout


def test_selftest_under_asan_and_ubsan(tmp_path):
    """The finiteness check, the table's builder, the planner and the loaders in a stand-alone executable with
    -fsanitize=address,undefined."""
    exe = _build_selftest(str(tmp_path / "depth_cut_selftest_san"),
                          ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"))
    out = subprocess.run([exe, SCENES], capture_output=True, text=True, timeout=300,
                         env=_env(ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert out.returncode == 0 and "all ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
