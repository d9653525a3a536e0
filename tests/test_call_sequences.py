"""What tests/test_gpu_call_sequences.py relies on, pinned on the CPU: the pool of tests/call_sequences.py holds frames of UNEQUAL
content, and every sequence takes a context through the stale-state conditions it is there for.  The counts are the oracle's; the
capacity of a stereo row list is the host planner's (tests/asan/plan_harness, as tests/test_plan_host.py reads its plan facts).  A
change to orbslam2_amd/synth.py, to the oracle or to the pool that makes two neighbouring frames alike fails here instead of
leaving the GPU sequences running without the conditions they were written for."""
import numpy as np
import pytest

from tests import call_sequences as S
from tests.test_plan_host import _line, run_harness

# sequence -> the conditions it must reach at least once (tests/call_sequences.py: conditions).  Every sequence whose frames are
# chosen here (parity, mixed, wide) has a level that empties, one that fills from zero and one that keeps a count above zero.
# Three sequences have their frames fixed by what they are about, and those frames cannot give all three: in shrink_grow a level
# stays equal only at zero (a slot that holds `flat` twice); in fewer_then_more no level rises from zero (its last call follows a
# sparser one only in slots that then hold `flat`); the two calls without a wait go from a full frame to a sparse or flat one in
# every slot, so nothing rises from zero and nothing stays equal.
EXPECT = {
    "shrink_grow": ("shrunk_to_zero", "level_emptied", "level_filled", "level_equal", "overflow_then_short", "short_then_overflow"),
    "fewer_then_more": ("shrunk_to_zero", "level_emptied", "level_equal", "level_equal_above_zero", "short_then_overflow", "stale_slot"),
    "parity": ("level_emptied", "level_filled", "level_equal", "level_equal_above_zero", "parity", "stale_slot"),
    "mixed": ("level_emptied", "level_filled", "level_equal", "level_equal_above_zero", "parity", "stale_slot"),
    "no_wait": ("shrunk_to_zero", "level_emptied", "overflow_then_short"),
    "wide": ("shrunk_to_zero", "level_emptied", "level_filled", "level_equal", "level_equal_above_zero", "overflow_then_short",
             "short_then_overflow"),
}


@pytest.fixture(scope="module")
def caps(tmp_path_factory):
    """sel_total (the CAPACITY of a slot, not a count) and row_cap of the plans the GPU module creates"""
    lines = [_line("s400/m%d" % mi, S.W, S.H, S.NF, mi=mi) for mi in (2, 8, 64)]
    out = {}
    for ln in run_harness(lines, tmp_path_factory.mktemp("plan")).stdout.splitlines():
        t = ln.split()
        if t and t[0] == "caps":
            out[t[1]] = {t[i]: int(t[i + 1]) for i in range(2, len(t), 2)}
    assert len(out) == 3 and len({tuple(sorted(c.items())) for c in out.values()}) == 1  # the same at every batch size
    return out["s400/m8"]


def test_pool_frames_are_unequal_and_keep_their_shape():
    R = S.refs()
    n = {key: len(r["kps"]) for key, r in R.items()}
    lv = {key: r["levels"] for key, r in R.items()}
    for side in (0, 1):
        assert 370 <= n["dense", side] <= S.NF and all(c > 0 for c in lv["dense", side][:7])   # the quota, on every level that has one
        assert 340 <= n["band", side] <= S.NF and all(c > 0 for c in lv["band", side][:7])
        assert 340 <= n["fallback", side] <= S.NF
        assert 15 <= n["cluster", side] <= 40 and max(lv["cluster", side]) <= 6      # a deep quadtree on few candidates
        assert 20 <= n["sparse", side] <= 80
        assert n["flat", side] == 0 and not any(len(c[0]) for c in R["flat", side]["cand"])
    assert lv["sparse", 0][0] == 0 and sum(lv["sparse", 0]) > 0                       # level 0 empty, others not
    assert len(R["cluster", 0]["cand"][0][0]) > 20 * lv["cluster", 0][0]             # many candidates per kept keypoint
    assert all(lv[key][S.NL - 1] == 0 for key in R)                                  # no quota on the last level at 400 features
    # cells that pass only at min_th_fast: scores below ini_th_fast (20) among the candidates, and cells that pass at once
    sc = np.concatenate([c[2] for c in R["fallback", 0]["cand"]])
    assert (sc < 20).mean() > 0.3 and (sc >= 20).any()
    # uRight / depth decide something on every textured pair; sparse and cluster match a few keypoints, flat none
    assert all(R[name, 0]["matches"] > 20 for name in S.TEXTURED)
    assert R["flat", 0]["matches"] == 0 and R["cluster", 0]["matches"] <= 20
    for name in S.FRAMES:  # real shifted views: no pair is two copies of one image, but for the constant one
        l, r, _ = S.pool()[name]
        assert np.array_equal(l, r) == (name == "flat")
    # no two images of the pool fill a level with the same candidates: a stale cell, candidate or keypoint of one is wrong for any other
    sig = {key: tuple(len(c[0]) for c in r["cand"]) for key, r in R.items() if key[0] != "flat"}
    assert len(set(sig.values())) == len(sig)


def test_row_lists_on_both_sides_of_the_capacity(caps):
    R = S.refs()
    assert caps["sel_total"] >= max(len(r["kps"]) for r in R.values())
    assert R["band", 1]["rows"].max() > caps["row_cap"]            # stereo_match_kernel scans every right keypoint
    for name in S.FRAMES:
        if name != "band":
            assert R[name, 1]["rows"].max() < caps["row_cap"], name
    assert R["dense", 1]["rows"].max() > 16                         # ... and dense rows are real lists, not empty ones


@pytest.mark.parametrize("name", sorted(S.SEQUENCES))
def test_sequences_reach_their_conditions(name, caps):
    got = S.conditions(S.SEQUENCES[name], caps["row_cap"])
    for c in EXPECT[name]:
        assert got[c], (name, c)
    print(name, {c: len(v) for c, v in got.items()})


def test_every_condition_is_reached_and_slots_change_between_calls(caps):
    reached = set()
    for name, steps in S.SEQUENCES.items():
        reached |= {c for c, v in S.conditions(steps, caps["row_cap"]).items() if v}
        for (_, a), (mode, b) in zip(steps, steps[1:]):  # no slot is given the image the call before gave it
            for i, (x, y) in enumerate(zip(a, b)):
                assert x != y or x[0] == "flat", (name, mode, i, x)
    assert reached == set(S.CONDITIONS)
    R = S.refs()
    for a, b in zip(S.PARITY, S.PARITY[1:]):  # every step's counts differ from the step before in the same slot
        for x, y in zip(a[1], b[1]):
            assert len(R[x]["kps"]) != len(R[y]["kps"]), (x, y)
