"""How the tests build and run the stand-alone drivers (tests/*_mirror/mirror_main.cpp) of the plain-C++ host forms under
orbslam2_amd/host/: one g++ line, built plain (-O2) or as an AddressSanitizer + UBSan program, and one way to run the program and to
judge its exit.  The programs are run directly; nothing is loaded into Python."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-O1", "-g"]
BUILDS = ["plain", "sanitized"]


def header(name):
    return os.path.join(ROOT, "orbslam2_amd", "host", name)


ABI_AND_CVMAT = ['#include "../../include/orbfe.h"', '#include "CvMat.h"']     # all that a host form includes of the project


def project_includes(path):
    """The #include "..." lines of a header."""
    return [ln for ln in open(path).read().splitlines() if ln.startswith('#include "')]


def build(tmp_path, mirror, build):
    """Compiles tests/<mirror>/mirror_main.cpp, `build` one of BUILDS; returns the program's path."""
    exe = str(tmp_path / ("mirror_" + build))
    src = os.path.join(ROOT, "tests", mirror, "mirror_main.cpp")
    flags = ["-O2"] if build == "plain" else SAN
    r = subprocess.run(["g++", "-std=c++14", "-Wall", "-Wextra", "-ffp-contract=off"] + flags + ["-o", exe, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run(exe, *args):
    """Runs the program; it must end with 0 and without a sanitizer report."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return r


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def bits_one_nan(a):
    """bits() with every NaN given one bit pattern: which payload and sign an arithmetic step leaves in a NaN is the processor's choice
    (x86 and gfx950 differ) and no part of the contract, which stores one pattern."""
    a = np.array(a)
    if a.dtype.kind == "f":
        a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])[np.isnan(a)] = {4: 0x7FC00000, 8: 0x7FF8000000000000}[a.dtype.itemsize]
    return bits(a)
