"""The split kernel's lobe-frame table on the CPU (scene_build.cpp lobe_frame_table): tests/lobe_frame_selftest.cpp holds which hit
records get an entry -- demo2's one plane and none of its spheres, a disk scene's plane and disk, all six face records of every box
of a box scene -- against the records' shape kinds and the YAML's shapes, checks the table's byte size (48 B a record) and that
FLUX_LOBE_FRAMES=0 yields no table.  The program is run once more as a stand-alone executable under AddressSanitizer and UBSan.
(The entries themselves are the device's work: tests/test_gpu_lobe_frames.py.)"""
import pytest

import selftest
from conftest import SCENES

CHECKS = ("demo2", "disk", "box", "switch")


def _build_selftest(exe, flags=()):
    return selftest.build(exe, "lobe_frame_selftest.cpp", csrc=("scene_build.cpp", "bvh.cpp", "launch_plan.cpp"), flags=flags)


@pytest.fixture(scope="module")
def selftest_out(tmp_path_factory):
    exe = _build_selftest(str(tmp_path_factory.mktemp("lobe") / "lobe_frame_selftest"))
    return selftest.run(exe, SCENES)


@pytest.mark.parametrize("name", CHECKS)
def test_which_records_get_an_entry(selftest_out, name):
    assert f"ok {name}" in selftest_out
    assert "all ok" in selftest_out


def test_selftest_under_asan_and_ubsan(tmp_path):
    """The host function, the scene build and the loaders compiled into a stand-alone executable with -fsanitize=address,undefined."""
    exe = _build_selftest(str(tmp_path / "lobe_frame_selftest_san"), selftest.SANITIZE)
    assert "all ok" in selftest.run(exe, SCENES, env=selftest.sanitize_env())
