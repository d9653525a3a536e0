"""The planner of OptimizeEssentialGraph (orbslam2_amd/csrc/orbfe_essential_plan.cpp) under AddressSanitizer + UBSan: a stand-alone
program (tests/asan/essential_plan_harness.cpp, built by tests/asan/essential_plan.mk, its own main; nothing is loaded into python) over chains, rings, covisibility bands,
duplicates, faulty indices and exact / too small capacities, walking every section of every blob."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_planner_under_asan_and_ubsan():
    d = os.path.join(ROOT, "tests", "asan")
    r = subprocess.run(["make", "-C", d, "-f", "essential_plan.mk", "essential_plan_harness"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(d, "essential_plan_harness")], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and r.stdout.startswith("essential plan ok 84"), r.stdout + r.stderr[-3000:]
