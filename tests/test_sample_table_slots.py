"""The glossy lobe's angle table (RenderParams::glossx), host side, on the CPU: tests/sample_tables_selftest.cpp builds host scenes
through flux_amd/csrc/scene_build.cpp and checks which slot every GlossyReflective hit record gets -- distinct 1 / (exponent + 1) bit
patterns in YAML order, duplicates sharing a slot, the cap of four, no table beside a non-unit plane normal -- and that DevHitRec
is still 96 B (the hit queue's slot count and the split kernel's 16 KiB rule depend on it)."""
import os

import pytest

import selftest


def build_selftest(out_dir):
    """(the program reads the library's internal headers, and a context's tables back through the HIP runtime)"""
    return selftest.build(os.path.join(str(out_dir), "sample_tables_selftest"), "sample_tables_selftest.cpp",
                          csrc=("scene_build.cpp", "bvh.cpp"), flags=("-L/opt/rocm/lib", "-lamdhip64"))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_selftest(tmp_path_factory.mktemp("sample_tables"))


def test_slot_assignment(exe):
    out = selftest.run(exe, "cpu")
    for name in ("record sizes", "no glossy record", "one exponent", "yaml order and duplicates", "two exponents", "cap",
                 "non-unit plane normal"):
        assert f"ok {name}" in out
    assert "all ok" in out
