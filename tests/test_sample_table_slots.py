"""The glossy lobe's angle table (RenderParams::glossx), host side, on the CPU: tests/sample_tables_selftest.cpp builds host scenes
through flux_amd/csrc/scene_build.cpp and checks which slot every GlossyReflective hit record gets -- distinct 1 / (exponent + 1) bit
patterns in YAML order, duplicates sharing a slot, the cap of four, no table beside a non-unit plane normal -- and that DevHitRec
is still 96 B (the hit queue's slot count and the split kernel's 16 KiB rule depend on it)."""
import os
import subprocess

import pytest

from conftest import ROOT


def build_selftest(out_dir):
    """Host-only clang (as tests/test_scene_build.py): the program reads the library's internal headers."""
    from flux_amd import build
    build.build_hip()
    exe = os.path.join(str(out_dir), "sample_tables_selftest")
    csrc = os.path.join(ROOT, "flux_amd", "csrc")
    subprocess.run(["/opt/rocm/llvm/bin/clang++", "-O2", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                    "-I/opt/rocm/include", "-pthread", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "sample_tables_selftest.cpp"),
                    os.path.join(csrc, "scene_build.cpp"), os.path.join(csrc, "bvh.cpp"),
                    "-L" + os.path.join(ROOT, "flux_amd"), "-lflux_hip", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + os.path.join(ROOT, "flux_amd"), "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    return build_selftest(tmp_path_factory.mktemp("sample_tables"))


def test_slot_assignment(selftest):
    out = subprocess.run([selftest, "cpu"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    for name in ("record sizes", "no glossy record", "one exponent", "yaml order and duplicates", "two exponents", "cap",
                 "non-unit plane normal"):
        assert f"ok {name}" in out.stdout
    assert "all ok" in out.stdout
