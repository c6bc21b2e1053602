"""When the split kernel's depth cut is admitted, on the CPU (launch_plan.cpp split_cut_depth, scene_build.cpp tput_products_finite):
tests/depth_cut_selftest.cpp holds the context's finiteness check against tables that are finite, tables with an infinite or a NaN
entry, and tables whose entries are finite while the bounce at the depth limit overflows; and the planner's answer for jobs with
and without the table, with the hit queue and with the ray queue, at depth 1, and under FLUX_SPLIT_DEPTH_CUT.  The program is run
once more as a stand-alone executable under AddressSanitizer and UBSan.  GPU side: tests/test_gpu_depth_cut.py."""
import pytest

import selftest
from conftest import SCENES

CHECKS = ("finite tables", "tables that are not finite", "plan")


def _build_selftest(exe, flags=()):
    """(-ffp-contract=off: the products are plain IEEE multiplications)"""
    return selftest.build(exe, "depth_cut_selftest.cpp", csrc=("scene_build.cpp", "bvh.cpp", "launch_plan.cpp"), flags=flags)


def test_admission(tmp_path):
    exe = _build_selftest(str(tmp_path / "depth_cut_selftest"))
    out = selftest.run(exe, SCENES)
    for name in CHECKS:
        assert f"ok {name}" in out
    assert "all ok" in out


def test_selftest_under_asan_and_ubsan(tmp_path):
    """The finiteness check, the table's builder, the planner and the loaders in a stand-alone executable with
    -fsanitize=address,undefined."""
    exe = _build_selftest(str(tmp_path / "depth_cut_selftest_san"), selftest.SANITIZE)
    assert "all ok" in selftest.run(exe, SCENES, env=selftest.sanitize_env())
