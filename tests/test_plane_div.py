"""The split kernel's unscaled first-plane division and the predicate its votes take (flux_amd/csrc/flux_plane_axis.h plane_div_unscaled,
plane_div_admits) on the CPU: tests/plane_div_selftest.cpp includes the header the host and the kernel share and
  - restates v_div_scale_f64's documented scaling rules and finds them idle for every den the predicate admits against every num of
    2^-894 <= |num| < 2^499 -- over a million random pairs and the exponent edges of both operands, on both sides of the predicate's floor
    and ceiling;
  - holds the function, seeded with the correctly rounded 1 / den moved by -2 .. +2 ulp, to num / den bit for bit over those pairs
    (|num| = 2e3 among them).  One exception, which the program spells out: a den whose fraction bits are all ones is the case in which
    the sequence's last step needs the correctly rounded reciprocal, which two Newton steps do not restore from a moved seed; there a
    moved seed is held to `/` only where they do restore it, the exact seed always.  (The kernel's own seed against the kernel's own `/`:
    tests/test_gpu_plane_div.py.)
  - holds both forms below 2^-764 -- the plane is missed either way -- for a num below the range, zeros and denormals among them.  Bit
    equality is NOT asserted there: a num of -0 gives +0 where `/` gives -0, and a denormal residual loses bits; the header argues why no
    guard is needed, and the program prints how many such pairs are bit-equal all the same;
  - holds the votes to the predicate on special values of d_a.
The program is run once more, on a tenth of the cases, as a stand-alone executable under AddressSanitizer and UBSan."""
import pytest

import selftest

CHECKS = ("predicate", "function", "small nums", "votes")


def _build(exe, flags=()):
    """(-ffp-contract=off, as the library's translation units: every fused multiply-add is spelled out)"""
    return selftest.build(exe, "plane_div_selftest.cpp", flags=flags)


@pytest.fixture(scope="module")
def selftest_out(tmp_path_factory):
    exe = _build(str(tmp_path_factory.mktemp("plane_div") / "plane_div_selftest"))
    return selftest.run(exe, timeout=600)


def test_unscaled_division_against_ieee(selftest_out):
    print(selftest_out)
    for name in CHECKS:
        assert f"ok {name}" in selftest_out
    assert "all ok" in selftest_out


def test_selftest_under_asan_and_ubsan(tmp_path):
    exe = _build(str(tmp_path / "plane_div_selftest_san"), selftest.SANITIZE)
    assert "all ok" in selftest.run(exe, "quick", env=selftest.sanitize_env(), timeout=600)
