"""The bump cursor and the staging layout of the host wrappers (orbslam2_amd/csrc/orbfe_arena.hpp) under AddressSanitizer + UBSan: a
stand-alone program (tests/asan/arena_harness.cpp, its own main; nothing is loaded into python).  For the alignment / minimum pairs of
the staging blocks, lba_carve and eg_carve: aligned fields that do not overlap, the same size with and without a base, zero counts at
their minimum, results before inputs, overflowing sizes refused, and every byte of every field written inside an allocation of exactly
the size the cursor reports."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_arena_under_asan_and_ubsan():
    d = os.path.join(ROOT, "tests", "asan")
    r = subprocess.run(["make", "-C", d, "arena_harness"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(d, "arena_harness")], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and r.stdout.startswith("arena ok "), r.stdout + r.stderr[-3000:]
