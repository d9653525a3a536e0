"""The launch planner of liborbfe.so (orbslam2_amd/csrc/orbfe_plan.cpp -- the translation unit the library links) run on the CPU
under AddressSanitizer + UBSan by tests/asan/plan_harness.cpp: the BASELINE geometries, the golden / natural-image sizes and a
seeded sweep of random geometries (drawn like tools/soak.py with SOAK_GEOM and SOAK_PATCH), each under the default plan and
every alternative knob set, at max_images 1, 2 and 128.  Every accepted plan must meet the coverage invariants the planner's
comments state, and every digest (status or error text, DeviceConfig bytes, per-level tables, each device table) must equal
tests/golden/plan_digests.json, which was recorded from orbfe_create before the planner was split out of it."""
import hashlib
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASAN_DIR = os.path.join(ROOT, "tests", "asan")
FIXTURE = os.path.join(ROOT, "tests", "golden", "plan_digests.json")

KNOB_SETS = ["-", "ORBFE_NO_INPLACE=1", "ORBFE_NO_PAIR=1,ORBFE_NO_TAIL=1", "ORBFE_NO_PAIR=0,ORBFE_NO_TAIL=0", "ORBFE_PYR_LDS=1",
             "ORBFE_NO_FUSE=1", "ORBFE_NO_PROC_ORDER=1", "ORBFE_OCTREE=1", "ORBFE_BLUR_RIDE_FROM=3"]
MAX_IMAGES = (1, 2, 128)
# name, width, height, nfeatures (8 levels, scale factor 1.2, FAST 20 / 7, patch 31, edge 19)
NAMED = [("tum", 640, 480, 1000), ("kitti", 1241, 376, 2000), ("euroc", 752, 480, 1200), ("d435", 1280, 720, 2500),
         ("golden", 320, 240, 500), ("golden400", 400, 160, 300), ("natural", 640, 427, 1000), ("natural624", 624, 427, 1000)]
N_RANDOM = 300


def _line(name, w, h, nf, sf=1.2, nl=8, ini=20, mn=7, hp=15, edge=19, knobs="-", mi=2):
    return "%s %d %d %d %.9g %d %d %d %d %d %d %d %s" % (name, w, h, nf, sf, nl, ini, mn, 2 * hp + 1, hp, edge, mi, knobs)


def named_cases():
    return [_line("%s/k%d/m%d" % (n, k, mi), w, h, nf, knobs=ks, mi=mi)
            for n, w, h, nf in NAMED for k, ks in enumerate(KNOB_SETS) for mi in MAX_IMAGES] + \
        [_line("kitti/capacity", 1241, 376, 2000, mi=30000)]  # more than 2^23 workgroups per launch: ORBFE_ERR_CAPACITY


def random_cases():
    out = []
    for i in range(N_RANDOM):
        rng = np.random.default_rng(9100 + i)
        w, h = int(rng.integers(120, 700)), int(rng.integers(100, 420))
        nf = int(rng.integers(50, 2500))
        ini = int(rng.integers(8, 45)); mn = int(rng.integers(3, ini + 1))
        sf, nl = float(np.float32(rng.uniform(1.04, 2.3))), int(rng.integers(1, 11))
        hp, edge = 15, 19
        if i % 2:
            hp = int(rng.integers(8, 19)); edge = max(19, hp + 4) + int(rng.integers(0, 4))
        out += [_line("r%d/k%d/m%d" % (i, k, mi), w, h, nf, sf, nl, ini, mn, hp, edge, ks, mi)
                for k, ks in enumerate(KNOB_SETS) for mi in MAX_IMAGES]
    return out


def _build():
    r = subprocess.run(["make", "-C", ASAN_DIR, "plan_harness"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(ASAN_DIR, "plan_harness")


def run_harness(lines, tmp_path, *extra):
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([_build(), str(cases)] + list(extra), capture_output=True, text=True, timeout=1200, env=env)
    assert r.returncode == 0 and "plan harness ok %d cases 0 violations" % len(lines) in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return r


def blocks(stdout):
    """case name -> the case's status / digest lines (what the fixture pins)"""
    out, cur = {}, None
    for ln in stdout.splitlines():
        if ln.startswith("case "):
            cur = ln.split()[1]
            out[cur] = []
        if cur and ln.split()[0] in ("case", "err", "cfg", "levels", "flags", "tab"):
            out[cur].append(ln)
    return out


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]


def test_planner_under_asan_matches_the_pre_split_digests(tmp_path):
    fix = json.load(open(FIXTURE))
    named = blocks(run_harness(named_cases(), tmp_path).stdout)
    assert {n: digest(b) for n, b in named.items()} == fix["named"]
    for n, b in named.items():  # every product geometry is planned at these batch sizes; 30000 KITTI images are refused
        assert b[0].endswith("rc 0") != (n == "kitti/capacity"), (n, b)
    assert named["kitti/capacity"][1] == "err max_images 30000: more than 2^23 workgroups per launch"
    rnd = blocks(run_harness(random_cases(), tmp_path).stdout)
    assert len(rnd) == N_RANDOM * len(KNOB_SETS) * len(MAX_IMAGES)
    assert digest([digest(b) for b in rnd.values()]) == fix["random_sweep"]
    accepted = sum(b[0].endswith("rc 0") for b in rnd.values())
    assert accepted > len(rnd) // 2
    assert not any("row map" in ln for b in rnd.values() for ln in b)  # the dr < 1 refusal is never reached


def test_host_trace_lines_are_unchanged(tmp_path):
    r = run_harness([_line("kitti_trace", 1241, 376, 2000, knobs="ORBFE_HOST_TRACE=1")], tmp_path)
    trace = [ln for ln in r.stderr.splitlines() if ln.startswith("orbfe: ")]
    assert len(trace) == 23 and digest(trace) == json.load(open(FIXTURE))["trace_kitti"], "\n".join(trace)


def facts(stdout):
    """case name -> the plan facts of its "facts" line (which blocks() leaves out of the digests): tail_first, tail_n,
    tail_max_images, pp_max_images, blur_ride_min_images, blur_ride_from, inplace_ok and levels {l: (rs_direct, rs_rw, pp_ok)}"""
    out = {}
    for ln in stdout.splitlines():
        t = ln.split()
        if t and t[0] == "facts":
            f = {t[i]: int(t[i + 1]) for i in range(2, 16, 2)}
            f["levels"] = {int(t[i][1:]): tuple(int(v) for v in t[i + 1].split(",")) for i in range(16, len(t), 2)}
            out[t[1]] = f
    return out


BIG = 1 << 30  # a threshold no batch reaches (ORBFE_NO_TAIL=0 / ORBFE_NO_PAIR=0: INT_MAX)
NO_TAIL = lambda f: f["tail_n"] == 0
TAIL3 = lambda f: f["tail_n"] == 3 and f["inplace_ok"] == 1 and f["levels"][1][0] == 1
LARGE_KNOB = {  # what each knob of the 32-pair rows of test_launch_plan_knobs_change_no_result changes
    "ORBFE_BLUR_RIDE_FROM=1": lambda f: f["blur_ride_from"] == 1 and f["blur_ride_min_images"] == 1 and f["inplace_ok"] == 1,
    "ORBFE_BLUR_RIDE_FROM=3": lambda f: f["blur_ride_from"] == 3 and f["blur_ride_min_images"] == 1 and f["inplace_ok"] == 1,
    "ORBFE_NO_FUSE=1": lambda f: f["inplace_ok"] == 1,
    "ORBFE_PYR_LDS=1": lambda f: not any(v[0] for v in f["levels"].values()) and f["inplace_ok"] == 0,
    "ORBFE_NO_TAIL=0": lambda f: f["tail_max_images"] >= BIG,
    "ORBFE_NO_PAIR=0": lambda f: f["pp_max_images"] >= BIG and f["levels"][1][2] == 1,
    "ORBFE_NO_INPLACE=1": lambda f: f["inplace_ok"] == 0,
}
# level 1 read in place and not paired: pyr_resize_blur_kernel<4, true, false> / pyr_resize_direct_kernel<4, true, false> below 64 images
UNPAIRED_IN_PLACE = lambda f: f["inplace_ok"] == 1 and f["levels"][1][0] == 1 and f["tail_first"] != 1 and not any(v[2] for v in f["levels"].values())


def gpu_plan_cases():
    """(harness line, the property the GPU case of the same geometry and knobs is there for)"""
    c = [(_line("tum1", 640, 480, 1000, mi=64), NO_TAIL), (_line("euroc", 752, 480, 1200, mi=64), NO_TAIL),
         (_line("d435i", 1280, 720, 2500, mi=64), NO_TAIL), (_line("kitti", 1241, 376, 2000, mi=128), TAIL3),
         (_line("w402", 402, 201, 600, mi=66), TAIL3), (_line("w403", 403, 202, 600, mi=64), TAIL3),
         (_line("w404", 404, 200, 600, mi=64), TAIL3), (_line("s400", 400, 200, 400, mi=130), TAIL3),
         (_line("s400_l3", 400, 200, 400, nl=3, mi=64), lambda f: (f["tail_first"], f["tail_n"], f["inplace_ok"]) == (1, 2, 0)),
         (_line("s400_sf26", 400, 200, 400, sf=2.6, nl=3, mi=64), lambda f: all(v[:2] == (0, 4) for v in f["levels"].values())),
         (_line("uhd_lds", 3840, 2160, 8000, knobs="ORBFE_PYR_LDS=1", mi=2),
          lambda f: [f["levels"][l][:2] for l in (1, 2)] == [(0, 2), (0, 2)])]
    for name, w, h, nf in [("s400", 400, 200, 400), ("tum1", 640, 480, 1000)]:
        c += [(_line("%s/%s" % (name, k), w, h, nf, knobs=k, mi=64), p) for k, p in LARGE_KNOB.items()]
    for name, w, h, nf, mi in [("kitti", 1241, 376, 2000, 6), ("tum1", 640, 480, 1000, 2)]:
        c += [(_line("%s/%s" % (name, k), w, h, nf, knobs=k, mi=mi), p) for k, p in
              [("ORBFE_NO_PAIR=1", UNPAIRED_IN_PLACE),
               ("ORBFE_NO_PAIR=1,ORBFE_BLUR_RIDE_FROM=0", lambda f: UNPAIRED_IN_PLACE(f) and f["blur_ride_from"] == 0)]]
    return c


def test_gpu_cases_run_the_plans_they_are_chosen_for(tmp_path):
    """The GPU tests of the batch-size-dependent plans (tests/test_gpu_plan_switches.py, the geometry sweep of
    tests/test_gpu_batch.py, the knob rows of tests/test_round4_entry_points.py, the 4K case of tests/test_gpu_sweep.py) each
    target a plan variant; a planner change that moves a case off its variant fails here instead of silently testing another."""
    cases = gpu_plan_cases()
    got = facts(run_harness([ln for ln, _ in cases], tmp_path).stdout)
    assert len(got) == len(cases)
    for ln, prop in cases:
        name = ln.split()[0]
        assert prop(got[name]), (name, got[name])
        if ln.split()[-1] == "-":  # the default thresholds: pairs and the tail up to 63 images, every blur in FAST's launch from 64
            f = got[name]
            assert (f["tail_max_images"], f["pp_max_images"], f["blur_ride_min_images"], f["blur_ride_from"]) == (63, 63, 64, 0), name
