"""The split kernel's f32 environment verdict (flux_amd/csrc/flux_env_verdict.h) on the CPU: tests/env_verdict_selftest.cpp includes the
kernel's own header and holds it against the exact predicate -- the signs of c = |o - p|^2 - r^2 and of g = |o + tb u - p|^2 - r^2 in
long double -- over a few million rays: never a wrong "wins" or "loses", every clear case of demo2's environment decided, and every
decided case one the f64 shortcut decides alike.  The program is run once more as a stand-alone executable under AddressSanitizer
and UBSan."""
import os
import subprocess

import pytest

from conftest import ROOT

CHECKS = ("random rays", "around the margins", "special distances", "cap")


def _build(exe, extra=()):
    """Host-only clang and -ffp-contract=off: the header spells out every fused multiply-add."""
    subprocess.run(["/opt/rocm/llvm/bin/clang++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", *extra, "-o", exe,
                    os.path.join(ROOT, "tests", "env_verdict_selftest.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def selftest_out(tmp_path_factory):
    exe = _build(str(tmp_path_factory.mktemp("env32") / "env_verdict_selftest"))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return out.stdout


def test_verdict_against_the_exact_predicate(selftest_out):
    for name in CHECKS:
        assert f"ok {name}" in selftest_out
    assert "all ok" in selftest_out


def test_selftest_under_asan_and_ubsan(tmp_path):
    exe = _build(str(tmp_path / "env_verdict_selftest_san"),
                 ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert out.returncode == 0 and "all ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
