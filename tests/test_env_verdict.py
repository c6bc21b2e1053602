"""The split kernel's f32 environment verdict (flux_amd/csrc/flux_env_verdict.h) on the CPU: tests/env_verdict_selftest.cpp includes the
kernel's own header and holds it against the exact predicate -- the signs of c = |o - p|^2 - r^2 and of g = |o + tb u - p|^2 - r^2 in
long double -- over a few million rays: never a wrong "wins" or "loses", every clear case of demo2's environment decided, and every
decided case one the f64 shortcut decides alike.  The program is run once more as a stand-alone executable under AddressSanitizer
and UBSan."""
import pytest

import selftest

CHECKS = ("random rays", "around the margins", "special distances", "cap")


def _build(exe, flags=()):
    """(-ffp-contract=off: the header spells out every fused multiply-add)"""
    return selftest.build(exe, "env_verdict_selftest.cpp", flags=flags)


@pytest.fixture(scope="module")
def selftest_out(tmp_path_factory):
    exe = _build(str(tmp_path_factory.mktemp("env32") / "env_verdict_selftest"))
    return selftest.run(exe)


def test_verdict_against_the_exact_predicate(selftest_out):
    for name in CHECKS:
        assert f"ok {name}" in selftest_out
    assert "all ok" in selftest_out


def test_selftest_under_asan_and_ubsan(tmp_path):
    exe = _build(str(tmp_path / "env_verdict_selftest_san"), selftest.SANITIZE)
    assert "all ok" in selftest.run(exe, env=selftest.sanitize_env(), timeout=600)
