"""Which branches of Frame::ComputeStereoMatches' tail (src/Frame.cc:596-641) the stereo inputs of the suite reach: CPU only.

tests/stereo_census.py restates the function in NumPy and counts every decision.  Here the restatement is held against the
oracle bit for bit on every input, each branch is required to be reached by at least one input (floors: conditions, not
measurements), the guards that cannot fire are shown not to fire, and the whole table is pinned in
tests/golden/stereo_tail_census.json so a change to synth or to an input cannot quietly take a branch out of reach.
tests/test_gpu_stereo_tail.py runs the same inputs through the HIP kernels.
"""
import json
import os

import numpy as np
import pytest

from tests import stereo_census as S

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def table():
    return {name: S.census_of(name) for name in S.INPUTS}


@pytest.mark.parametrize("name", list(S.INPUTS))
def test_restatement_equals_oracle(table, name):
    """Three-way agreement, CPU leg: the NumPy restatement and orc_stereo_matches read the reference the same way."""
    ur, dp, u2, d2, c = table[name]
    what = "%s (%s)" % (name, S.INPUTS[name][2])
    assert len(ur) == c["n_left"]
    bad = np.nonzero((ur != u2) | (dp != d2))[0]
    assert bad.size == 0, "%s: restatement and oracle differ at keypoints %s: u_right %s vs %s, depth %s vs %s" % (
        what, bad[:5].tolist(), u2[bad[:5]].tolist(), ur[bad[:5]].tolist(), d2[bad[:5]].tolist(), dp[bad[:5]].tolist())
    assert c["matched"] == int((ur >= 0).sum()) == c["accepted"] - c["cut"]
    assert c["nvdi"] == c["accepted"]
    # a surviving clamp is visible in the outputs: depth = bf / 0.01f, uRight = (float)((double)uL - 0.01) < uL
    bf = np.float32(S.INPUTS[name][0]["bf"])
    if bf != 0:
        assert int((dp == bf / np.float32(0.01)).sum()) == c["clamp_surviving"], what


def _counters(table):
    return {name: v[4] for name, v in table.items()}


FLOORS = {
    "disparity < 0": lambda c: c["disparity_negative"] >= 100,
    "disparity < 0 next to accepted matches that survive": lambda c: c["disparity_negative"] >= 100 and c["matched"] >= 100,
    "disparity >= maxD": lambda c: c["disparity_ge_maxd"] >= 10,
    "disparity == maxD exactly": lambda c: c["disparity_eq_maxd"] >= 1,
    "best candidate exactly at uL - maxD": lambda c: c["best_at_min_u"] >= 5,
    "best candidate exactly at uL": lambda c: c["best_at_max_u"] >= 100,
    "accepted SAD equal to a non-zero 1.5 * 1.4 * median": lambda c: c["sad_at_threshold"] >= 1 and c["median"] > 0,
    "clamp taken and surviving the median cut": lambda c: c["clamp_surviving"] >= 10,
    "clamp taken, erased by a median of 0": lambda c: c["clamp"] >= 10 and c["median"] == 0 and c["clamp_surviving"] == 0,
    "median == 0 with >= 100 accepted: all cut": lambda c: c["median"] == 0 and c["accepted"] >= 100 and c["cut"] == c["accepted"] and c["matched"] == 0,
    "nvdi == 0 with >= 50 left keypoints": lambda c: c["nvdi"] == 0 and c["n_left"] >= 50 and c["median"] is None,
    "delta_r == 0.5": lambda c: c["delta_half"] >= 5,
    "SAD tie": lambda c: c["sad_tie"] >= 5,
    "Hamming tie for the best candidate": lambda c: c["hamming_tie"] >= 50,
    "Q12 guard": lambda c: c["q12_guard"] >= 1,
    "bestincR == +-L": lambda c: c["best_inc_at_end"] >= 100,
    # vDistIdx[size / 2]: the upper median of an even count, the middle of an odd one, the only element of one
    "odd nvdi below 16 with a cut": lambda c: c["nvdi"] < 16 and c["nvdi"] % 2 == 1 and c["nvdi"] > 1 and c["cut"] >= 1,
    "even nvdi below 16": lambda c: 0 < c["nvdi"] < 16 and c["nvdi"] % 2 == 0,
    "nvdi == 1": lambda c: c["nvdi"] == 1 and c["matched"] == 1,
}


@pytest.mark.parametrize("branch", list(FLOORS))
def test_reachability_floors(table, branch):
    hit = [name for name, c in _counters(table).items() if FLOORS[branch](c)]
    assert hit, "no census input reaches: " + branch


def test_new_inputs_reach_what_they_were_built_for(table):
    c = _counters(table)
    assert c["noisy_copy"]["disparity_negative"] >= 100 and c["roll_plus1"]["disparity_negative"] >= 100
    for name in ("maxd_11.5", "maxd_27.75", "maxd_61"):
        assert c[name]["disparity_ge_maxd"] >= 10, name
    for name in ("composite5", "composite6", "composite7"):
        assert c[name]["clamp_surviving"] >= 10, name
    assert c["identical"]["median"] == 0 and c["identical"]["accepted"] >= 100 and c["identical"]["matched"] == 0
    assert c["bf0"]["coarse"] == 0 and c["bf0"]["n_left"] >= 500 and c["bf0"]["n_right"] >= 500
    assert c["right_flat"]["n_right"] == 0 and c["right_flat"]["n_left"] >= 500


def test_dead_branches(table):
    """Three guards of the reference cannot fire; the census shows it on every input instead of chasing them.

    deltaR (src/Frame.cc:604-607).  The SAD minimum is the FIRST strict minimum of the 11 distances and is not at an end, so
    d1 > d2 and d3 >= d2 (d1 = left neighbour, d2 = minimum, d3 = right neighbour).  Then the denominator
    2 (d1 + d3 - 2 d2) = 2 ((d1 - d2) + (d3 - d2)) > 0, and |d1 - d3| <= (d1 - d2) + (d3 - d2) puts deltaR in [-0.5, 0.5];
    -0.5 would need d1 == d2, so deltaR is in (-0.5, 0.5].  Every operand is an integer below 121 * 510 < 2^17 and every
    intermediate below 2^19, so the float arithmetic up to the division is exact: `deltaR < -1 || deltaR > 1` never holds and the
    denominator is never 0.  The edge that exists is deltaR == 0.5 exactly (d3 == d2), which periodic patterns produce.

    endu >= cols (:577) and a band that ends right of the level (cr + 10 >= cols).  The candidate filter only passes
    uR <= uL, rounding is monotonic, so scaleduR0 <= scaleduL, and the left keypoint lies >= 19 px inside its level
    (EDGE_THRESHOLD): scaleduR0 + 11 <= cols - 19 + 11 < cols.
    """
    for name, c in _counters(table).items():
        assert c["delta_denominator_zero"] == 0 and c["delta_outside_unit"] == 0, name
        assert c["band_right_of_level"] == 0, name
        if c["delta_min"] is not None:
            assert -0.5 < c["delta_min"] <= c["delta_max"] <= 0.5, name
        assert c["sad_max"] <= 121 * 510, name
        assert c["delta_half"] <= c["sad_tie"], name  # deltaR == 0.5 is d3 == d2: a SAD tie
    assert max(c["delta_max"] or 0 for c in _counters(table).values()) == 0.5


def test_pinned_counts(table):
    """The recomputed census equals tests/golden/stereo_tail_census.json exactly (python -m tests.stereo_census rewrites it)."""
    with open(os.path.join(HERE, "golden", S.GOLDEN)) as f:
        golden = json.load(f)
    got = json.loads(json.dumps(_counters(table)))
    assert sorted(got) == sorted(golden)
    for name in got:
        diff = {k: (got[name][k], golden[name].get(k)) for k in got[name] if got[name][k] != golden[name].get(k)}
        assert not diff and sorted(got[name]) == sorted(golden[name]), "%s: (recomputed, pinned) %s" % (name, diff)


def test_census_of_the_existing_inputs_is_on_record():
    with open(os.path.join(HERE, "golden", S.GOLDEN)) as f:
        golden = json.load(f)
    for name in ("kitti", "small", "euroc", "777x333", "131x97", "checker24_roll9", "q12"):
        assert S.INPUTS[name][2].startswith("existing input") and golden[name]["n_left"] > 0
    # what the existing inputs never reached, and why the new ones are there
    for name in ("kitti", "small", "euroc", "777x333", "131x97", "checker24_roll9"):
        g = golden[name]
        assert g["disparity_negative"] == g["clamp"] == g["disparity_ge_maxd"] == 0 and g["median"] > 0
