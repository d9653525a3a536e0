"""The two FAST launches of the split plan (orbfe_fast_launches in orbslam2_amd/csrc/orbfe_plan.cpp, the function run_chain calls)
on the CPU under AddressSanitizer + UBSan, through tests/asan/fast_split_harness.cpp, which prints every launch as
fast_cell_kernel decodes it from DeviceConfig::fast_cell_c0 / fast_blur_t0.  For the BASELINE and golden geometries, 1 / 2 / 8
levels and 200 random geometries, and for every first riding blur level a call can have (every ORBFE_BLUR_RIDE_FROM value
included): the two launches' (cell, blur tile) sets are disjoint, their union is exactly the single launch's set, neither launch
has an empty grid, and a one-level pyramid never splits."""
import os
import subprocess

import numpy as np

from tests.test_plan_host import ASAN_DIR, NAMED, ROOT, _line

CSRC = os.path.join(ROOT, "orbslam2_amd", "csrc")
N_RANDOM = 200


def cases():
    out = []
    for n, w, h, nf in NAMED:  # the BASELINE geometries and the golden / natural-image sizes
        for nl in (1, 2, 8):
            out.append(_line("%s/l%d" % (n, nl), w, h, nf, nl=nl, mi=128))
    for k in range(0, 10):  # the knob moves the plan's first riding level: the ranges themselves come from what a call passes
        out.append(_line("kitti/ride%d" % k, 1241, 376, 2000, knobs="ORBFE_BLUR_RIDE_FROM=%d" % k, mi=128))
    out += [_line("kitti/nofuse", 1241, 376, 2000, knobs="ORBFE_NO_FUSE=1", mi=128), _line("kitti/split0", 1241, 376, 2000, knobs="ORBFE_FAST_SPLIT=0", mi=128),
            _line("kitti/split1", 1241, 376, 2000, knobs="ORBFE_FAST_SPLIT=1", mi=128), _line("tum/l1/split1", 640, 480, 1000, nl=1, knobs="ORBFE_FAST_SPLIT=1", mi=2)]
    for i in range(N_RANDOM):  # drawn like the random sweep of tests/test_plan_host.py
        rng = np.random.default_rng(77100 + i)
        w, h = int(rng.integers(120, 700)), int(rng.integers(100, 420))
        nf = int(rng.integers(50, 2500))
        ini = int(rng.integers(8, 45)); mn = int(rng.integers(3, ini + 1))
        sf, nl = float(np.float32(rng.uniform(1.04, 2.3))), int(rng.integers(1, 11))
        hp, edge = 15, 19
        if i % 2:
            hp = int(rng.integers(8, 19)); edge = max(19, hp + 4) + int(rng.integers(0, 4))
        out.append(_line("r%d" % i, w, h, nf, sf, nl, ini, mn, hp, edge, "-", int(rng.choice([1, 2, 128]))))
    return out


def run(lines, tmp_path):
    exe = str(tmp_path / "fast_split_harness")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fno-fast-math",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe,
                        os.path.join(ASAN_DIR, "fast_split_harness.cpp"), os.path.join(CSRC, "orbfe_plan.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    cases_file = tmp_path / "cases.txt"
    cases_file.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(cases_file)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "fast split harness ok %d cases 0 violations" % len(lines) in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return r.stdout


def launch_set(c0, c1, t0, t1):
    return {("cell", c) for c in range(c0, c1)} | {("tile", t) for t in range(t0, t1)}


def test_split_launches_partition_the_single_launch(tmp_path):
    out = run(cases(), tmp_path)
    plans, n_lines, n_split, accepted = {}, 0, 0, 0
    for ln in out.splitlines():
        t = ln.split()
        if t[0] == "plan":
            plans[t[1]] = {t[i]: int(t[i + 1]) for i in range(2, len(t), 2)}
            accepted += 1
        if t[0] != "launches":
            continue
        assert "UNENCODABLE" not in ln, ln
        P = plans[t[1]]
        side_blur, bf = int(t[3]), int(t[5])
        single = [int(v) for v in t[7:11]]
        k = int(t[12])
        parts = [[int(v) for v in t[13 + 4 * j:17 + 4 * j]] for j in range(k)]
        n_lines += 1
        # the single launch: every cell, the blur tiles of the levels from blur_first on
        assert single[:2] == [0, P["cells"]] and single[3] == P["tiles"] and 0 <= single[2] <= P["tiles"], ln
        assert (bf == 0) <= (single[2] == 0) and (bf == P["nlevels"]) <= (single[2] == P["tiles"]), ln
        if P["nlevels"] == 1:
            assert k == 1, ln
        splittable = P["nlevels"] >= 2 and 0 < P["cut"] < P["cells"]
        assert k == (2 if splittable else 1), ln
        if k == 1:
            assert parts[0] == single, ln
            continue
        n_split += 1
        a, b = (launch_set(*p) for p in parts)
        assert a and b and not (a & b) and (a | b) == launch_set(*single), ln
        for p in parts:  # the grid of a launch: workgroups of four cells, then of four tiles, per image
            assert (max(0, p[1] - p[0]) + 3) // 4 + (max(0, p[3] - p[2]) + 3) // 4 > 0, ln
        # the side launch is level 0: its cells, and its blur tiles exactly when they ride aside
        assert parts[0][:2] == [0, P["cut"]], ln
        assert max(0, parts[0][3] - parts[0][2]) == (P["tcut"] if side_blur else 0), ln
    assert accepted > N_RANDOM // 2 and n_split > n_lines // 2
    # the planner's threshold: never for one level or ORBFE_FAST_SPLIT=0, every batch for =1, else not below the plan's
    # blur_ride_min_images, the batch from which every blur rides
    for name, P in plans.items():
        if P["nlevels"] < 2 or name == "kitti/split0":
            assert P["min_images"] == 2 ** 31 - 1, name
        elif name == "kitti/split1":
            assert P["min_images"] == 1, name
        else:
            assert P["min_images"] >= P["ride_min"], name
            if not name.startswith("kitti/ride"):  # no knob: the default threshold of the riding blur
                assert P["min_images"] >= P["ride_min"] == 64, name
