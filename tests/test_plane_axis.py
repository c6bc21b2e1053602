"""The split kernel's reduced first-plane test for an axis-aligned stored normal (flux_amd/csrc/flux_plane_axis.h) on the CPU:
tests/plane_axis_selftest.cpp includes the header the host and the kernel share and holds num = p_a - o_a, den = d_a and their quotient
against the general dot products in every order and fusion of their terms -- over three million random rays and the full grid of special
values (zeros, subnormals, 1e-300, 1, 1e300, infinities, NaN) in every component of the ray, for the six axis normals with zeros of either
sign: bit-equal wherever the predicate admits the ray, the predicate refusing every ray of the grid for which a form differs, the
kernel's f32 vote implying the predicate, and the classifier.  The program is run once more, on a tenth of the cases, as a stand-alone
executable under AddressSanitizer and UBSan."""
import pytest

import selftest

CHECKS = ("classifier", "random rays", "special values")


@pytest.fixture(scope="module")
def selftest_out(tmp_path_factory):
    """(-ffp-contract=off: the program spells out every fused multiply-add)"""
    exe = selftest.build(str(tmp_path_factory.mktemp("plane_axis") / "plane_axis_selftest"), "plane_axis_selftest.cpp")
    return selftest.run(exe, timeout=600)


def test_reduced_form_against_every_general_form(selftest_out):
    print(selftest_out)
    for name in CHECKS:
        assert f"ok {name}" in selftest_out
    assert "all ok" in selftest_out


def test_selftest_under_asan_and_ubsan(tmp_path):
    exe = selftest.build(str(tmp_path / "plane_axis_selftest_san"), "plane_axis_selftest.cpp", flags=selftest.SANITIZE)
    assert "all ok" in selftest.run(exe, "quick", env=selftest.sanitize_env(), timeout=600)
