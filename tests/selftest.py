"""The one way a test compiles and runs a stand-alone tests/*_selftest.cpp.

Host-only clang by default: plain g++ cannot compile flux_device.h's ext_vector_type records.  -ffp-contract=off as the library's
(flux_amd/build.py): the programs restate its host arithmetic, where a fused multiply-add would be another result."""
import os
import subprocess

import switches
from conftest import ROOT

CLANG = "/opt/rocm/llvm/bin/clang++"
FLAGS = ("-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-Wall")
# a sanitized build is the same stand-alone executable, run directly under sanitize_env()
SANITIZE = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer")


def sanitize_env(**more):
    return switches.clean_env(ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1", **more)


def build(exe, source, csrc=(), host=False, flags=(), compiler=CLANG):
    """tests/<source> compiled as `exe`.  With the files `csrc` of flux_amd/csrc, or host=True, the program is linked: those files,
    the C++ host layer and the built library."""
    cmd = [compiler, *FLAGS, "-o", exe, os.path.join(ROOT, "tests", source)]
    if csrc or host:
        from flux_amd import build as lib_build
        lib_build.build_hip()
        lib = os.path.join(ROOT, "flux_amd")
        cmd += ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", *[os.path.join(lib, "csrc", s) for s in csrc],
                *[os.path.join(lib, "host", s) for s in lib_build.HOST_SOURCES],
                "-L" + lib, "-lflux_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd + list(flags), check=True)
    return exe


def run(exe, *args, env=None, stdin=None, timeout=300):
    """The program's stdout.  It must exit with status 0 and report nothing a sanitizer prints; env=None: no switch of the library set."""
    out = subprocess.run([exe, *args], input=stdin, capture_output=True, text=True, timeout=timeout,
                         env=switches.clean_env() if env is None else env)
    tail = out.stdout[-3000:] + out.stderr[-4000:]
    assert out.returncode == 0, tail
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, tail
    return out.stdout
