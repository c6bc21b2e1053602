"""The split kernel's reduced first-plane test for an axis-aligned stored normal (flux_amd/csrc/flux_plane_axis.h) on the CPU:
tests/plane_axis_selftest.cpp includes the header the host and the kernel share and holds num = p_a - o_a, den = d_a and their quotient
against the general dot products in every order and fusion of their terms -- over three million random rays and the full grid of special
values (zeros, subnormals, 1e-300, 1, 1e300, infinities, NaN) in every component of the ray, for the six axis normals with zeros of either
sign: bit-equal wherever the predicate admits the ray, the predicate refusing every ray of the grid for which a form differs, the
kernel's f32 vote implying the predicate, and the classifier.  The program is run once more, on a tenth of the cases, as a stand-alone
executable under AddressSanitizer and UBSan."""
import os
import subprocess

import pytest

from conftest import ROOT

CHECKS = ("classifier", "random rays", "special values")


def _build(exe, extra=()):
    """Host-only clang and -ffp-contract=off: the test spells out every fused multiply-add."""
    subprocess.run(["/opt/rocm/llvm/bin/clang++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-Wall", *extra, "-o", exe,
                    os.path.join(ROOT, "tests", "plane_axis_selftest.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def selftest_out(tmp_path_factory):
    exe = _build(str(tmp_path_factory.mktemp("plane_axis") / "plane_axis_selftest"))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return out.stdout


def test_reduced_form_against_every_general_form(selftest_out):
    print(selftest_out)
    for name in CHECKS:
        assert f"ok {name}" in selftest_out
    assert "all ok" in selftest_out


def test_selftest_under_asan_and_ubsan(tmp_path):
    exe = _build(str(tmp_path / "plane_axis_selftest_san"),
                 ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"))
    out = subprocess.run([exe, "quick"], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert out.returncode == 0 and "all ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
