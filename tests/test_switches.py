"""The library's environment switches (flux_amd/csrc/flux_switches.h) on the CPU: tests/switches_selftest.cpp sets every variable to
unset, "", "0", "1", "-3", "abc", "7x" and the accessor's own edge values and prints what the accessor answers; the expected column
below was written by hand from the expressions the call sites held before the header existed (atoi: "abc" and "" read as 0, "7x" as
7).  The program is run once more as a stand-alone executable under AddressSanitizer and UBSan.  And the names are stated three
times -- the header, tests/switches.py, DESIGN.md's table -- and nowhere else does the library read the environment."""
import os
import re

import pytest

import selftest
import switches
from conftest import ROOT

CSRC = os.path.join(ROOT, "flux_amd", "csrc")
INPUTS = ("unset", "[]", "[0]", "[1]", "[-3]", "[abc]", "[7x]")
# "set and atoi() == 0 means off"
OFF = dict(zip(INPUTS, "0110010"))
EXPECTED = {name: OFF for name in ("FLUX_SAMPLE_TABLES", "FLUX_THROUGHPUT_TABLE", "FLUX_LOBE_FRAMES", "FLUX_PLANE_AXIS", "FLUX_SAMPLE_ORDER",
                                   "FLUX_SPLIT_DEPTH_CUT", "FLUX_SPLIT_UNIFORM_A")}
# min(cap, max(0, atoi) & ~1u), cap = 110
EXPECTED["FLUX_SPLIT_HITQ_CAP"] = dict(zip(INPUTS + ("[67]", "[-5]", "[110]", "[200]"), "110 0 0 0 0 0 6 66 0 110 110".split()))
# max(1, min(64, atoi)) replaces H = 46
EXPECTED["FLUX_SPLIT_HITQ_TAKE_AT"] = dict(zip(INPUTS + ("[64]", "[100]"), "46 1 1 1 1 1 7 64 64".split()))
# atoi replaces the caller's default, 3
EXPECTED["FLUX_DENOISE_LDS_LEVELS"] = dict(zip(INPUTS + ("[8]",), "3 0 0 1 -3 0 7 8".split()))
# max(1, atoi), then 1..16; unset: the hardware's, in 1..16
EXPECTED["FLUX_BUILD_THREADS"] = dict(zip(INPUTS + ("[16]", "[99]"), "hardware 1 1 1 1 1 7 16 16".split()))
# the value as it stands
EXPECTED["FLUX_RCCL_LIB"] = dict(zip(INPUTS + ("[/opt/lib/librccl.so]",), ("(null)", "", "0", "1", "-3", "abc", "7x", "/opt/lib/librccl.so")))


def _check(stdout):
    got = {}
    for line in stdout.splitlines()[:-1]:
        name, value, result = line.split(" ", 2)
        got.setdefault(name, {})[value] = result
    hardware = got["FLUX_BUILD_THREADS"]["unset"]
    assert 1 <= int(hardware) <= 16
    got["FLUX_BUILD_THREADS"]["unset"] = "hardware"
    assert got == EXPECTED
    assert stdout.splitlines()[-1] == "all ok"


def test_every_accessor_parses_as_its_call_site_did(tmp_path):
    _check(selftest.run(selftest.build(str(tmp_path / "switches_selftest"), "switches_selftest.cpp")))


def test_selftest_under_asan_and_ubsan(tmp_path):
    exe = selftest.build(str(tmp_path / "switches_selftest_san"), "switches_selftest.cpp", flags=selftest.SANITIZE)
    _check(selftest.run(exe, env=selftest.sanitize_env()))


def test_the_names_are_the_same_everywhere():
    header = open(os.path.join(CSRC, "flux_switches.h")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("## Environment switches"):]
    section = section[:section.index("\n## ", 1)]
    in_design = re.findall(r"^\| `(FLUX_[A-Z0-9_]+)`", section, flags=re.M)
    assert set(re.findall(r'"(FLUX_[A-Z0-9_]+)"', header)) == set(switches.NAMES) == set(in_design)
    assert len(switches.NAMES) == len(set(switches.NAMES)) == len(in_design)


def test_no_other_file_of_the_library_reads_the_environment():
    readers = [f for f in sorted(os.listdir(CSRC)) if "getenv" in open(os.path.join(CSRC, f), errors="replace").read()]
    assert readers == ["flux_switches.h"]


def test_a_name_that_is_no_switch_is_refused(monkeypatch):
    with pytest.raises(KeyError):
        switches.set_switches(monkeypatch, FLUX_SPLIT_HITQ_CAPS=0)
    assert switches.queue(None) == {} and switches.queue((66, 2)) == {"FLUX_SPLIT_HITQ_CAP": 66, "FLUX_SPLIT_HITQ_TAKE_AT": 2}
    monkeypatch.setenv("FLUX_SAMPLE_ORDER", "0")
    assert not any(n in switches.clean_env(FLUX_BUILD_THREADS=None) for n in switches.NAMES)
    assert switches.clean_env(FLUX_BUILD_THREADS=1)["FLUX_BUILD_THREADS"] == "1"
