"""The split kernel's throughput product table (flux_plan.h tput_index, scene_build.cpp build_tput_table) and the hit queue's slot on
the CPU: tests/throughput_table_selftest.cpp holds every table entry of demo2 and of a 16-record scene against the product the
kernel's loop forms (bit patterns), checks the index of (n, ml), the slot's field offsets and which jobs get a table, and prints the
launch planner's answer for the shipped scenes, whose every reported field is pinned here.  The program is run once more as a
stand-alone executable under AddressSanitizer and UBSan."""
import pytest

import selftest
from conftest import SCENES

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


def _build_selftest(exe, flags=()):
    """(-ffp-contract=off: the products are plain IEEE multiplications)"""
    return selftest.build(exe, "throughput_table_selftest.cpp", csrc=("scene_build.cpp", "bvh.cpp", "launch_plan.cpp"), flags=flags)


@pytest.fixture(scope="module")
def selftest_out(tmp_path_factory):
    exe = _build_selftest(str(tmp_path_factory.mktemp("tput") / "throughput_table_selftest"))
    return selftest.run(exe, SCENES)


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
    exe = _build_selftest(str(tmp_path / "throughput_table_selftest_san"), selftest.SANITIZE)
    assert "all ok" in selftest.run(exe, SCENES, env=selftest.sanitize_env())
