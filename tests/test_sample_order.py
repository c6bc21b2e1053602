"""The split kernel's per-set sample order (flux_amd/csrc/flux_sample_order.h) on the CPU: tests/sample_order_selftest.cpp includes the
header the table build and the kernel share and is held here to an independent numpy restatement (tests/sample_order_ref.py) -- the
deal is a bijection whose quarters are the kernel's slices and whose 64-aligned batches are sorted groups where N is a multiple of 256,
the key clamps NaN, infinities and +-1 into range, equal keys keep index order.  The program's own checks (random and adversarial key
arrays: the row is a permutation whatever the keys are) run once plain and once as a stand-alone executable under AddressSanitizer
and UBSan."""
import numpy as np
import pytest

import sample_order_ref as ref
import selftest
from selftest import run as _run

SIZES = (64, 81, 256, 289, 4225, 16384)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return selftest.build(str(tmp_path_factory.mktemp("sample_order") / "sample_order_selftest"), "sample_order_selftest.cpp")


def _ints(text):
    return np.array(text.split(), dtype=np.int64)


@pytest.mark.parametrize("N", SIZES)
def test_deal_is_a_bijection_on_the_kernels_slices(exe, N):
    row = _ints(_run(exe, "deal", str(N)))  # equal keys: the sorted sequence is 0 .. N-1, the row is the deal itself
    assert row.shape == (N,) and np.array_equal(np.sort(row), np.arange(N))
    assert np.array_equal(row, ref.row_from_keys(np.zeros(N, dtype=np.int64)))
    lo = _ints(_run(exe, "slices", str(N)))
    assert list(lo) == [N * q // 4 for q in range(5)]
    for K in (1, 2, 4):  # render_split_kernel: s_lo = N sub / K
        for sub in range(K + 1):
            assert N * sub // K == lo[sub * (4 // K)]
    if N % 256 == 0:
        for K in (1, 2, 4):
            for sub in range(K):
                for b in range(N * sub // K, N * (sub + 1) // K, 64):
                    assert row[b] % 64 == 0 and np.array_equal(row[b:b + 64], row[b] + np.arange(64))
        # group g sits in quarter g mod 4, the quarters filled front to back
        assert np.array_equal(row[::64] // 64, np.concatenate([np.arange(q, N // 64, 4) for q in range(4)]))


def test_key_clamps_every_value_into_range(exe):
    vals = ["nan", "-nan", "inf", "-inf", "1", "-1", "0", "-0", "1e300", "-1e300", "0.984375", "0.98437499", "-0.984375", "0.5", "4e-324",
            "0x1.fffffffffffffp-1", "-0x1.fffffffffffffp-1"]
    pairs = [(a, b) for a in vals for b in vals]
    keys = _ints(_run(exe, "keys", stdin="\n".join(f"{a} {b}" for a, b in pairs)))
    x = np.array([float.fromhex(a) if "0x" in a else float(a) for a, _ in pairs])
    y = np.array([float.fromhex(b) if "0x" in b else float(b) for _, b in pairs])
    assert keys.min() >= 0 and keys.max() < 1 << 14
    assert np.array_equal(keys, ref.key(x, y))
    k = dict(zip(pairs, keys))
    assert k[("nan", "nan")] == 0 and k[("-inf", "-1")] == 0 and k[("inf", "1")] == (1 << 14) - 1
    assert k[("1", "-1")] == 0x1555 and k[("nan", "inf")] == 0x2aaa


def test_equal_keys_keep_index_order(exe):
    rng = np.random.default_rng(7)
    for N in (81, 256, 289):
        for keys in (rng.integers(0, 4, N), rng.integers(0, 1 << 14, N), np.full(N, 9)):
            row = _ints(_run(exe, "row", stdin="\n".join(str(int(v)) for v in keys)))
            assert np.array_equal(np.sort(row), np.arange(N))
            assert np.array_equal(row, ref.row_from_keys(keys))
            sorted_idx = row[ref.deal_positions(N)]  # the sorted sequence: the row at the positions of rank 0, 1, ...
            same = keys[sorted_idx][1:] == keys[sorted_idx][:-1]
            assert np.all(keys[sorted_idx][1:] >= keys[sorted_idx][:-1]) and np.all(sorted_idx[1:][same] > sorted_idx[:-1][same])


def test_selftest_checks(exe):
    out = _run(exe)
    for name in ("keys", "deal", "rows"):
        assert f"ok {name}" in out
    assert "all ok" in out


def test_selftest_under_asan_and_ubsan(tmp_path):
    exe = selftest.build(str(tmp_path / "sample_order_selftest_san"), "sample_order_selftest.cpp", flags=selftest.SANITIZE)
    assert "all ok" in _run(exe, "quick", env=selftest.sanitize_env(), timeout=600)
