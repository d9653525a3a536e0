"""Which decisions of the seven projection matchers (tests/matcher_census.py lists them) the inputs of the suite reach: CPU only.

The literal transcriptions (oracle/literal_matchers.py, oracle/literal_kf_matchers.py) count every decision of their loops.  Here
they are held against the C oracle exactly on every input; every decision is required to be reached by at least one input
(FLOORS: conditions, not measurements); the branches that cannot be reached are shown not to be; the whole table is pinned in
tests/golden/matcher_census.json; the tie inputs are shown to tell the reference's `first minimum in GetFeaturesInArea order` from
two wrong orders; and the overflow input is shown to exceed the first size of the device's candidate list.
tests/test_gpu_matcher_census.py runs the same inputs through the HIP entry points.
"""
import json
import os

import numpy as np
import pytest

from oracle import literal_kf_matchers as LK
from oracle import literal_matchers as LM
from tests import matcher_census as MC

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def table():
    return {(name, m): MC.census_of(name, m) for name, m in MC.CASES}


@pytest.mark.parametrize("name,matcher", MC.CASES)
def test_literal_equals_oracle(table, name, matcher):
    """Three-way agreement, CPU leg: the instrumented literal transcription and the C oracle read the reference the same way."""
    (ref, nref), (got, ngot), c = table[(name, matcher)]
    what = "%s / %s (%s)" % (name, matcher, MC.INPUTS[name][2])
    bad = np.nonzero(ref != got)[0]
    assert ngot == nref and bad.size == 0, "%s: count %d vs %d; differ at %s: literal %s, oracle %s" % (
        what, ngot, nref, bad[:5].tolist(), got[bad[:5]].tolist(), ref[bad[:5]].tolist())
    # the counters add up to what the function returned
    if matcher in ("last", "kf"):
        assert nref == c["accepted"] - c["rot_rejected"], what
    elif matcher == "by_sim3":
        assert nref == c["sim3_mutual"] == int((ref >= 0).sum()), what
        assert c["accepted"] >= c["sim3_mutual"] + c["sim3_one_direction_only"] + c["sim3_mutual_disagree"], what  # `accepted`: both directions
    else:
        assert nref == c["accepted"], what
    assert c["accepted_on_tie"] == c["tie_one_cell"] + c["tie_one_column"] + c["tie_columns_lower_index_later"] + c["tie_columns_other"], what


def _counters(table):
    return {key: v[2] for key, v in table.items()}


def _ge(key, n):
    return lambda c: c[key] >= n


def _frame_bounds(c):
    """A row of `last` or `points`: the image test is Frame's, on its float bounds (the keyframe-side rows use IsInImage)."""
    return c["motion_forward"] + c["motion_backward"] + c["motion_neither"] + c["in_view"] > 0


# Conditions, not measurements: reject-type gates want 10 points, each kind of tie 5 accepted matches, each single-sided bound 1.
FLOORS = {
    "point invalid": _ge("invalid", 10),
    "z < 0": _ge("z_negative", 10),
    "z < 0 where the function does not test it, and the point projects into the image": _ge("z_negative_in_image", 10),
    "z == 0: a non-finite projection that falls out at the image test": lambda c: c["z_zero"] >= 1 and c["out_left"] + c["out_right"] >= c["z_zero"],
    "left of the image (float bounds)": lambda c: c["out_left"] >= 1 and _frame_bounds(c),
    "right of the image (float bounds)": lambda c: c["out_right"] >= 1 and _frame_bounds(c),
    "above the image (float bounds)": lambda c: c["out_top"] >= 1 and _frame_bounds(c),
    "below the image (float bounds)": lambda c: c["out_bottom"] >= 1 and _frame_bounds(c),
    "too near": _ge("too_near", 10),
    "too far": _ge("too_far", 10),
    "too near next to points that pass": lambda c: c["too_near"] >= 10 and c["accepted"] >= 10,
    "too far next to points that pass": lambda c: c["too_far"] >= 10 and c["accepted"] >= 10,
    "viewing cosine": _ge("view_cos", 10),
    "predicted level clamped at nlevels - 1": _ge("level_clamped_high", 10),
    "radius of a point seen head-on": _ge("radius_small", 1),
    "empty window": _ge("window_empty", 10),
    "window clipped at the left edge of the grid": _ge("window_clipped_left", 1),
    "window clipped at the right edge": _ge("window_clipped_right", 1),
    "window clipped at the top edge": _ge("window_clipped_top", 1),
    "window clipped at the bottom edge": _ge("window_clipped_bottom", 1),
    "candidate below the level window": _ge("cand_below_level", 10),
    "candidate above the level window": _ge("cand_above_level", 10),
    "mvuRight radius gate": _ge("cand_uright_gate", 10),
    "stereo chi-square above 7.8": _ge("cand_chi2_stereo", 10),
    "mono chi-square above 5.99": _ge("cand_chi2_mono", 10),
    "keypoint matched on entry": _ge("cand_matched_on_entry", 10),
    "keypoint taken by an earlier point of the call": _ge("cand_taken_in_call", 10),
    "every candidate skipped or gated": _ge("no_candidate_left", 10),
    "best distance above the threshold": _ge("best_above_threshold", 10),
    "ratio rule": _ge("ratio_rejected", 10),
    "ratio rule not applied: best and second best on different levels": _ge("ratio_other_level", 1),
    "rotation histogram": _ge("rot_rejected", 10),
    "forward": _ge("motion_forward", 1),
    "backward": _ge("motion_backward", 1),
    "neither forward nor backward": _ge("motion_neither", 1),
    "Observations() == 0: a keypoint matched twice, both counted": _ge("double_count", 10),
    "SearchBySim3: found in one direction only": _ge("sim3_one_direction_only", 10),
    "SearchBySim3: the two directions disagree": _ge("sim3_mutual_disagree", 10),
    "accepted": _ge("accepted", 10),
    "accepted on a tie, tied keypoints in one cell": _ge("tie_one_cell", 5),
    "accepted on a tie, in two cells of one column": _ge("tie_one_column", 5),
    "accepted on a tie, in two columns, the lower keypoint index in the later column": _ge("tie_columns_lower_index_later", 5),
}
# the same gates behind the keyframe's truncated integer bounds
KF_FLOORS = {"left": "out_left", "right": "out_right", "above": "out_top", "below": "out_bottom"}


@pytest.mark.parametrize("branch", list(FLOORS))
def test_reachability_floors(table, branch):
    hit = [key for key, c in _counters(table).items() if FLOORS[branch](c)]
    assert hit, "no census input reaches: " + branch


@pytest.mark.parametrize("side", list(KF_FLOORS))
def test_reachability_floors_keyframe_bounds(table, side):
    hit = [key for key, c in _counters(table).items() if MC.build(key[0])["keyframe"] and c[KF_FLOORS[side]] >= 1]
    assert hit, "no keyframe-bounds input has a point " + side


@pytest.mark.parametrize("matcher", MC.MATCHERS)
def test_every_matcher_meets_the_new_gates(table, matcher):
    """What the issue found missing is reached through EVERY function that has the decision, not through one of them."""
    mine = [c for (name, m), c in _counters(table).items() if m == matcher]
    total = lambda key: sum(c[key] for c in mine)
    assert total("accepted_on_tie") >= 5 and total("tie_winner_not_lowest_index") >= 5
    assert total("tie_one_cell") >= 1 and total("tie_one_column") >= 1 and total("tie_columns_lower_index_later") >= 1
    if matcher == "kf":  # no test of the depth's sign in this overload
        assert total("z_negative_in_image") >= 10
    else:
        assert total("z_negative") >= 10
    if matcher != "last":  # no distance range in the last-frame matcher
        assert total("too_near") >= 10 and total("too_far") >= 10 and total("level_clamped_high") >= 10


def test_dead_branches(table):
    """Two decisions cannot be reached; the census shows it on every input instead of chasing them.

    Window wholly outside the grid (the four early returns of GetFeaturesInArea, src/Frame.cc:342-356, src/KeyFrame.cc:568-582).
    Every function opens its window at a projection (u, v) that has passed its image test, mnMinX <= u <= mnMaxX, with r > 0.
    nMinCellX >= 64 needs (u - mnMinX - r) * 64 / (mnMaxX - mnMinX) >= 64, i.e. u - r >= mnMaxX; nMaxCellX < 0 needs
    u + r <= mnMinX - (a cell).  Neither holds for u inside the bounds; the same in y.  A keyframe truncates its bounds towards
    zero: for mnMinX <= 0 (every bound of this suite, and of any camera whose undistorted corners lie outside the image) that
    moves the lower bound up by less than 1 and leaves u - (int)mnMinX - r < mnMaxX - mnMinX for r >= 1.

    Predicted level clamped at 0 (MapPoint::PredictScale, src/MapPoint.cc:385-417).  nScale = ceil(log(mfMaxDistance / dist) /
    log 1.2) < 0 needs mfMaxDistance / dist < 1 / 1.2, i.e. dist > 1.2 mfMaxDistance -- and every function that predicts a level
    has turned such a point away as too far (dist > 1.2f * mfMaxDistance) just before.  Only float rounding at
    dist == 1.2 mfMaxDistance could let one through, an input the census does not construct.  The clamp at nlevels - 1 is alive:
    it is reached for dist in [0.8 mfMinDistance, mfMinDistance).
    """
    for key, c in _counters(table).items():
        assert c["window_outside_grid"] == 0, key
        assert c["level_clamped_low"] == 0, key
        assert c["tie_columns_other"] == 0 or key[0] not in ("tie", "tie_wide"), key  # the tie inputs arrange indices against the order


def test_pinned_counts(table):
    """The recomputed census equals tests/golden/matcher_census.json exactly (python -m tests.matcher_census rewrites it)."""
    with open(os.path.join(HERE, "golden", MC.GOLDEN)) as f:
        golden = json.load(f)
    got = {"%s/%s" % key: c for key, c in _counters(table).items()}
    assert sorted(got) == sorted(golden)
    for name in got:
        diff = {k: (got[name][k], golden[name].get(k)) for k in got[name] if got[name][k] != golden[name].get(k)}
        assert not diff and sorted(got[name]) == sorted(golden[name]), "%s: (recomputed, pinned) %s" % (name, diff)


def test_census_of_the_existing_inputs_is_on_record():
    """What the scenes the suite had never reached, and why the new ones are there: no point behind the camera or on its plane, none
    outside its distance range, and not one accepted match that a Hamming tie decided -- while points outside the image, shared
    window minima above the threshold and every other gate were there."""
    with open(os.path.join(HERE, "golden", MC.GOLDEN)) as f:
        golden = json.load(f)
    rows = [(name, m) for name, m in MC.CASES if name in MC.EXISTING]
    assert len(rows) >= 14 and {"fuse_40", "fuse_41", "fuse_42", "sim3_50", "sim3_51", "sim3_52", "sim3_53", "kfbounds_71"} <= set(MC.EXISTING)
    for name, m in rows:
        g = golden["%s/%s" % (name, m)]
        assert g["accepted"] > 100, (name, m)
        assert g["z_negative"] == g["z_zero"] == g["z_below_half"] == g["z_negative_in_image"] == 0, (name, m)
        assert g["too_near"] == g["too_far"] == 0, (name, m)
        assert g["accepted_on_tie"] == 0 and g["double_count"] == 0, (name, m)
        assert g["out_left"] + g["out_right"] + g["out_top"] + g["out_bottom"] >= 5, (name, m)
    assert sum(golden["%s/%s" % key]["window_min_shared"] for key in rows) >= 50  # ties were there, above the threshold
    assert max(golden["%s/%s" % key]["ratio_rejected"] for key in rows) == 0
    assert max(golden["%s/%s" % key]["sim3_mutual_disagree"] for key in rows) == 0


# ------------------------------------------------------------------ two wrong tie rules, stated next to the right one
class _LowestIndexFrame(LM.Frame):
    """`Ties go to the lowest keypoint index`: the window's keypoints in index order instead of GetFeaturesInArea's."""

    def get_features_in_area(self, *a, **kw):
        return sorted(super().get_features_in_area(*a, **kw))


class _LowestIndexKeyFrame(LK.KeyFrame):
    def GetFeaturesInArea(self, *a, **kw):
        return sorted(super().GetFeaturesInArea(*a, **kw))


class _RowMajorFrame(LM.Frame):
    """`Ties go in cell-y-major order`: the cells walked row by row (iy, then ix, then index) -- an ix / iy swap in the candidate key."""

    def get_features_in_area(self, *a, **kw):
        return sorted(super().get_features_in_area(*a, **kw), key=lambda j: (self.cell[j][1], self.cell[j][0], j))


class _RowMajorKeyFrame(LK.KeyFrame):
    def GetFeaturesInArea(self, *a, **kw):
        return sorted(super().GetFeaturesInArea(*a, **kw), key=lambda j: (self.cell[j][1], self.cell[j][0], j))


VARIANTS = {"lowest keypoint index": (_LowestIndexFrame, _LowestIndexKeyFrame), "cell-y-major": (_RowMajorFrame, _RowMajorKeyFrame)}


@pytest.mark.parametrize("matcher", MC.MATCHERS)
@pytest.mark.parametrize("name", ["tie", "tie_wide"])
def test_the_tie_inputs_tell_the_reference_order_from_two_wrong_ones(table, name, matcher):
    """On the tie inputs the oracle's answer differs from a resolver that breaks ties by keypoint index and from one that walks the
    cells row-major, for every matcher: a HIP key with such an order cannot pass tests/test_gpu_matcher_census.py."""
    (ref, nref), _, c = table[(name, matcher)]
    s, p = MC.build(name), MC.INPUTS[name][1][matcher]
    assert c["accepted_on_tie"] >= 5
    for what, (frame_cls, kf_cls) in VARIANTS.items():
        var, _ = MC.literal_run(matcher, s, p, None, frame_cls, kf_cls)
        differ = int((var != ref).sum())
        print("%s / %s: `%s` differs from the oracle at %d entries" % (name, matcher, what, differ))
        assert differ >= 3, (name, matcher, what)
    if name == "tie_wide":  # every bit of the candidate key's fields: keypoint indices above 32768, cells beyond 32 both ways
        m = ref[ref >= 0] if matcher not in ("last", "points", "kf") else np.nonzero(ref >= 0)[0]
        assert (m > 32768).sum() >= 5 and len(s["k"]) < 65535
        cells = [LM.Frame(s["k"], s["d"], None, s["bounds"], MC.CAMT, s["sf"]).cell[int(j)] for j in m if j >= len(s["k"]) - s["n_clusters"]]
        assert sum(1 for cx, cy in cells if cx >= 32 and cy >= 32) >= 3 and sum(1 for cx, cy in cells if cx < 32 and cy < 32) >= 3


@pytest.mark.parametrize("matcher", ["fuse", "sim3_projection", "last", "points", "kf"])
def test_the_overflow_input_exceeds_the_first_candidate_list(matcher):
    """The device sizes its candidate list at 64 per query on a context's first call (run_window_queries, orbfe_match.hip); the
    windows of this input, counted by the oracle's grid with the level window the entry point hands to the device, hold more."""
    s, p = MC.build("overflow"), MC.INPUTS["overflow"][1][matcher]
    sizes, nq = MC.window_sizes(matcher, s, p)
    print("%s: %d queries, %d windows, %d candidates, largest %d" % (matcher, nq, len(sizes), sum(sizes), max(sizes)))
    assert sum(sizes) > 64 * nq
    assert max(sizes) > 256 and min(sizes) == 0 and sum(1 for n in sizes if n == 0) >= 10
