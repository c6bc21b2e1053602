"""The split kernel's hit queue on the CPU: tests/hitq_pool_selftest.cpp asks the launch planner for the five shipped scenes' plans
-- the array-of-structures pool keeps the bytes, the hit-queue / ray-queue decision and the reported fields the field-major queue had
-- and checks the pool's arithmetic (flux_plan.h, the functions the kernel's pass loop calls): entries lie inside the pool, clear of
each other, and phase A is never admitted with less than 64 * 68 B free, for every pool size from the floor to the cap."""
import pytest

import selftest
from conftest import SCENES

# scene, sample root -> kernel, TYP, C, H, bits per bounce, waves per pixel, LDS of the queues per wave.  The values of the field-major
# queue: C slots of 68 B (demo2 at 16384 spp: 110, H = 46), or the 5120-byte ray queue (glass: a dielectric's weight is not in its record;
# one wave a pixel at 256 spp: fewer than 96 slots fit beside demo2's records)
PLANS = {
    ("demo1", 16): (2, 1, 100, 36, 3, 1, 100 * 68), ("demo1", 128): (2, 1, 114, 50, 3, 4, 114 * 68),
    ("demo2", 16): (2, 1, 0, 0, 0, 1, 5120), ("demo2", 128): (2, 1, 110, 46, 4, 4, 110 * 68),
    ("disk_light", 16): (2, 0, 0, 0, 0, 1, 5120), ("disk_light", 128): (2, 0, 110, 46, 4, 4, 110 * 68),
    ("box_room", 16): (2, 0, 0, 0, 0, 1, 5120), ("box_room", 128): (2, 0, 110, 46, 5, 4, 110 * 68),
    ("glass", 16): (2, 0, 0, 0, 0, 1, 5120), ("glass", 128): (2, 0, 0, 0, 0, 4, 5120),
}


@pytest.fixture(scope="module")
def selftest_out(tmp_path_factory):
    exe = selftest.build(str(tmp_path_factory.mktemp("hitq_pool") / "hitq_pool_selftest"), "hitq_pool_selftest.cpp",
                         csrc=("scene_build.cpp", "bvh.cpp"))
    return selftest.run(exe, SCENES)


def test_pool_arithmetic(selftest_out):
    for name in ("plans", "room test"):
        assert f"ok {name}" in selftest_out
    assert "all ok" in selftest_out


def test_shipped_scenes_keep_their_plans(selftest_out):
    got = {}
    for line in selftest_out.splitlines():
        if line.startswith("plan "):
            w = line.split()
            f = dict(kv.split("=") for kv in w[2:])
            got[(w[1], int(f["root"]))] = tuple(int(f[k]) for k in ("kernel", "typ", "hq_cap", "hq_th", "hq_bits", "K",
                                                                    "queue_bytes_per_wave"))
    assert got == PLANS
