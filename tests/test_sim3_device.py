"""The geometric matchers of LoopClosing::ComputeSim3 on device-resident keyframes: orbfe_enqueue_search_by_sim3 (ORBmatcher::SearchBySim3,
src/ORBmatcher.cc:1098-1322; orbslam2_amd/csrc/orbfe_sim3_device.hip) and orbfe_enqueue_search_by_projection_sim3
(SearchByProjection(pKF, Scw, vpPoints, vpMatched, th), :285-398; orbfe_match_device.hip).  Every comparison is exact: against the C
oracle and against the synchronous entry point (orbfe_search_by_sim3 / orbfe_search_by_projection_sim3) on the same arrays.

The inputs are the census inputs of tests/matcher_census.py plus the "crowd" scenes built here: the projection matcher keeps the FOUR
smallest statically admissible keys of a window and scans the window again when all four were taken by earlier points of the call
(resolve_kernel, TOPK = 4).  No census input has a point that is ACCEPTED after such a rescan, so a wrong rescan would go unseen; a
crowd is nine copies of one map point over nine near-identical keypoints, which take them one after another -- the fifth copy and
every later one finds its four best keys taken and is accepted on a fifth.  The CPU tests pin what the inputs reach.

Device arrays, guards and the stream follow tests/test_fuse_device.py: inputs over-allocated by PAD zero entries, outputs between
GUARD sentinel cells, never the default stream; a check the kernels miss reads inside the test's own allocation.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import literal_kf_matchers as LK
from oracle import oracle as O
from tests import matcher_census as MC
from tests.device_arrays import Guarded, context, upload
from tests.test_fuse_device import CELLS, PAD, _Kf, _kf_of, _Table
from tests.test_gpu_matcher_census import hip_run

NAMES = ["orbfe_enqueue_search_by_sim3", "orbfe_enqueue_search_by_projection_sim3"]
PROJ_INPUTS = [name for name, v in MC.INPUTS.items() if "sim3_projection" in v[1]]
BYSIM3_INPUTS = [name for name, v in MC.INPUTS.items() if "by_sim3" in v[1]]
TOPK = 4  # the prefix resolve_kernel keeps per query (orbfe_match_device.hip)
CROWD = 8  # copies of the point and of its keypoint: nine of each with the originals, more than TOPK + 4
CROWD_COUNTS = {"tie": 72, "sim3_51": 605}  # accepted matches of the crowd scenes (pinned from the builder below)


# ------------------------------------------------------------------ crowd scenes
def crowd_scene(name):
    """The census input `name` with a crowd: an accepted point i0 and the keypoint m0 it got; CROWD more rows of the point at the end of
    the table; CROWD more keypoints at m0's place (x shifted by hundredths of a pixel, the octave kept, not matched on entry), copy j
    holding the point's descriptor with j + 1 random bits flipped."""
    s, p = dict(MC.build(name)), MC.INPUTS[name][1]["sim3_projection"]
    ref, _ = MC.oracle_run("sim3_projection", s, p)
    i0 = int(np.nonzero(ref >= 0)[0][0])
    m0 = int(ref[i0])
    rng = np.random.default_rng(77)
    rep = lambda a, i: np.concatenate([a, np.repeat(a[i:i + 1], CROWD, axis=0)])
    for key in ("pos", "normal", "max_d", "min_d", "desc", "valid"):
        s[key] = rep(s[key], i0)
    k = rep(s["k"], m0)
    k["x"][-CROWD:] += 0.01 * (1 + np.arange(CROWD, dtype=np.float32))
    d = rep(s["d"], m0)
    for j in range(CROWD):
        bits = np.zeros(256, bool)
        bits[rng.choice(256, j + 1, replace=False)] = True
        d[len(d) - CROWD + j] = s["desc"][i0] ^ np.packbits(bits, bitorder="little")
    s.update(k=k, d=d, ur=np.concatenate([s["ur"], np.full(CROWD, -1.0, np.float32)]),
             kf_matched=np.concatenate([s["kf_matched"], np.zeros(CROWD, np.uint8)]))
    return s, p


_CROWDS = {}


def crowd(name):
    if name not in _CROWDS:
        _CROWDS[name] = crowd_scene(name)
    return _CROWDS[name]


class _Tap:
    """points["valid"] of the literal transcription, remembering the query it was last asked about."""

    def __init__(self, v):
        self.v, self.last = v, -1

    def __len__(self):
        return len(self.v)

    def __getitem__(self, i):
        self.last = i
        return self.v[i]


def accepted_beyond_the_prefix(s, p):
    """(oracle result, literal result, queries accepted after their TOPK smallest statically admissible keys were all taken while more
    existed).  The keys of a window are ordered by (distance, GetFeaturesInArea order) and filtered for the level band and kf_matched,
    which is what window_topk_kernel keeps; `taken` is the state of vpMatched when the query has its turn."""
    tap, log = _Tap(s["valid"]), []

    class Logging(LK.KeyFrame):
        def GetFeaturesInArea(self, x, y, r, census=None, levels=None):
            v = super().GetFeaturesInArea(x, y, r, census, levels)
            log.append((tap.last, list(v), levels))
            return v

    lit = MC.literal_run("sim3_projection", dict(s, valid=tap), p, kf_cls=Logging)
    ref = MC.oracle_run("sim3_projection", s, p)
    taken = s["kf_matched"].astype(bool).copy()
    beyond = []
    for q, vidx, (lo, hi) in log:
        octv = s["k"]["octave"]
        static = [(int(np.unpackbits(s["desc"][q] ^ s["d"][i]).sum()), pos, i) for pos, i in enumerate(vidx)
                  if lo <= octv[i] <= hi and not s["kf_matched"][i]]
        static.sort()
        if len(static) > TOPK and all(taken[i] for _, _, i in static[:TOPK]) and lit[0][q] >= 0:
            beyond.append(q)
        if lit[0][q] >= 0:
            taken[lit[0][q]] = True
    return ref, lit, beyond


# ------------------------------------------------------------------ CPU
def test_the_library_exports_the_calls():
    from orbslam2_amd import api
    L = api.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "orbfe.h")).read()
    for name in NAMES:
        assert name in api.EXPORTS and ("int %s(" % name) in header
        fn = getattr(L, name)  # AttributeError: the symbol is not exported
        args = [0 if t is C.c_int else 0.0 if t is C.c_float else None for t in fn.argtypes]
        assert fn(*args) == api.ERR_INVALID, name
    for m in ("enqueue_search_by_sim3", "enqueue_search_by_projection_sim3"):
        assert callable(getattr(api.Context, m))


def test_the_census_inputs_decide_something():
    """Summed over the inputs that have the matcher, the decisions the kernels restate go both ways (the pinned table of
    tests/test_matcher_census.py)."""
    table = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", MC.GOLDEN)))
    assert PROJ_INPUTS == ["sim3_50", "sim3_51", "kfbounds_71", "among", "retreat", "among_kfbounds", "tie", "tie_wide", "overflow"]
    assert BYSIM3_INPUTS == ["among", "retreat", "among_kfbounds", "sideways", "tie", "tie_wide"]
    total = lambda matcher, names, key: sum(table["%s/%s" % (name, matcher)][key] for name in names)
    for key in ("cand_matched_on_entry", "cand_taken_in_call", "no_candidate_left", "best_above_threshold", "accepted_on_tie",
                "tie_winner_not_lowest_index"):
        assert total("sim3_projection", PROJ_INPUTS, key) > 0, key
    assert total("sim3_projection", ("tie", "tie_wide"), "accepted_on_tie") == 70
    for key in ("sim3_mutual", "sim3_one_direction_only", "sim3_mutual_disagree", "accepted_on_tie"):
        assert total("by_sim3", BYSIM3_INPUTS, key) > 0, key
    assert table["sideways/by_sim3"]["sim3_mutual_disagree"] == 33 == total("by_sim3", BYSIM3_INPUTS, "sim3_mutual_disagree")
    # the two keyframes of SearchBySim3 differ in size; a slot and a query count that do not fill the last workgroup of four waves
    scenes = [MC.build(name) for name in BYSIM3_INPUTS]
    assert any(len(s["k1"]) != len(s["k"]) for s in scenes)
    assert any(len(s["k1"]) % 4 for s in scenes) and any(len(s["k"]) % 4 for s in scenes)
    assert any(len(MC.build(name)["pos"]) % 4 for name in PROJ_INPUTS)
    s = MC.build("tie_wide")
    assert len(s["k"]) > 32768
    assert MC.oracle_run("sim3_projection", s, MC.INPUTS["tie_wide"][1]["sim3_projection"])[0].max() > 32768
    assert MC.oracle_run("by_sim3", s, MC.INPUTS["tie_wide"][1]["by_sim3"])[0].max() > 32768


@pytest.mark.parametrize("name", sorted(CROWD_COUNTS))
def test_a_crowd_is_accepted_beyond_the_four_key_prefix(name):
    s, p = crowd(name)
    ref, lit, beyond = accepted_beyond_the_prefix(s, p)
    assert ref[1] == lit[1] == CROWD_COUNTS[name] and np.array_equal(ref[0], lit[0])
    assert len(beyond) >= 4, beyond
    # the copies take successive keypoints one after another
    n_pts, nk = len(s["pos"]), len(s["k"])
    got = ref[0][n_pts - CROWD:]
    assert (got >= 0).all() and len(set(got.tolist())) == CROWD and set(beyond) >= set(range(n_pts - CROWD + TOPK, n_pts))
    assert (got >= nk - CROWD).sum() >= CROWD - 1  # the original point took one keypoint of the nine


def test_no_census_input_is_accepted_beyond_the_prefix():
    """Why the crowds exist: sim3_50 is the only plain input with queries whose four best keys are all taken while more exist, and
    none of them ends in an accepted match."""
    for name in ("sim3_50", "sim3_51", "tie"):
        s, p = MC.build(name), MC.INPUTS[name][1]["sim3_projection"]
        assert accepted_beyond_the_prefix(s, p)[2] == [], name


# ------------------------------------------------------------------ helpers (GPU)
@pytest.fixture(scope="module")
def gpu():
    import torch
    from orbslam2_amd import api
    ctx = context(api)
    assert np.array_equal(ctx.tables()["scale"], O.Extractor().scale_factors())
    yield api, ctx, torch.cuda.Stream()
    ctx.close()


def _pts_dev(pts):
    pos, mx, mn, d, ok = pts
    return [upload(np.ascontiguousarray(pos, np.float32).reshape(-1), pad=PAD)[0], upload(np.ascontiguousarray(mx, np.float32), pad=PAD)[0], upload(np.ascontiguousarray(mn, np.float32), pad=PAD)[0],
            upload(np.ascontiguousarray(d, np.uint8).reshape(-1), pad=PAD)[0], upload(np.ascontiguousarray(ok, np.int32), pad=PAD)[0]]


class _Pair:
    """The two keyframes of a by_sim3 scene in HBM with their map points, uploaded and bucketed once."""

    def __init__(self, api, ctx, st, s):
        self.s = s
        self.kf1 = _Kf(api, ctx, st, s["k1"], s["d1"], None, s["bounds"], s["keyframe"])
        self.kf2 = _Kf(api, ctx, st, s["k"], s["d"], None, s["bounds"], s["keyframe"])
        self.p1, self.p2 = _pts_dev(s["pts1"]), _pts_dev(s["pts2"])

    def enqueue(self, ctx, th, out, st, rec1=None, rec2=None, p1=None, p2=None):
        s = self.s
        ctx.enqueue_search_by_sim3(rec1 or self.kf1.rec, s["T_last"], [t.data_ptr() for t in self.p1] if p1 is None else p1,
                                   rec2 or self.kf2.rec, s["T_cur"], [t.data_ptr() for t in self.p2] if p2 is None else p2,
                                   s["s12"], s["R12"], s["t12"], th, *out.ptrs(), stream=st.cuda_stream)


class _Out12:
    """match12[n1], count, status between guards."""

    def __init__(self, n1):
        self.n = n1
        self.match, self.count, self.status = Guarded.cells(n1), Guarded.cells(1), Guarded.cells(1)

    def ptrs(self):
        return [g.ptr for g in (self.match, self.count, self.status)]

    def fetch(self):
        return self.match.fetch(), int(self.count.fetch()[0]), int(self.status.fetch()[0])

    def check(self, ref, nref, what):
        m, count, status = self.fetch()
        bad = np.nonzero(m != ref)[0]
        assert status == 0, (what, status)
        assert count == nref and bad.size == 0, "%s: count %d vs %d; differ at %s: device %s, reference %s" % (
            what, count, nref, bad[:8].tolist(), m[bad[:8]].tolist(), ref[bad[:8]].tolist())


class _OutProj:
    """pt_match[n_pts], kf_match[n], count, status between guards."""

    def __init__(self, n_pts, n):
        self.n_pts, self.n = n_pts, n
        self.pt, self.kf, self.count, self.status = Guarded.cells(n_pts), Guarded.cells(n), Guarded.cells(1), Guarded.cells(1)

    def ptrs(self):
        return [g.ptr for g in (self.pt, self.kf, self.count, self.status)]

    def fetch(self):
        return self.pt.fetch(), self.kf.fetch(), int(self.count.fetch()[0]), int(self.status.fetch()[0])

    def check(self, ref, nref, what):
        pt, kf, count, status = self.fetch()
        bad = np.nonzero(pt != ref)[0]
        assert status == 0, (what, status)
        assert count == nref and bad.size == 0, "%s: count %d vs %d; differ at %s: device %s, reference %s" % (
            what, count, nref, bad[:8].tolist(), pt[bad[:8]].tolist(), ref[bad[:8]].tolist())
        inverse = np.full(self.n, -1, np.int32)
        hit = np.nonzero(ref >= 0)[0]
        inverse[ref[hit]] = hit
        assert len(set(ref[hit].tolist())) == len(hit) == nref  # a keypoint is taken at most once
        assert np.array_equal(kf, inverse), "%s: d_kf_match is not the inverse of d_pt_match" % what


def _enqueue_proj(ctx, rec, s, table, d_valid, d_matched, th, out, st, n_pts=None, d_index=None):
    ctx.enqueue_search_by_projection_sim3(rec, s["Scw"], table.n if n_pts is None else n_pts, 0 if d_index is None else d_index.data_ptr(), table.n,
                                          *table.ptrs(), d_valid.data_ptr(), 0 if d_matched is None else d_matched.data_ptr(), th, *out.ptrs(),
                                          stream=st.cuda_stream)


def _run_projection(gpu, s, p, what):
    import torch
    api, ctx, st = gpu
    ref, nref = MC.oracle_run("sim3_projection", s, p)
    sref, snref = hip_run(ctx, "sim3_projection", s, p)
    assert snref == nref and np.array_equal(sref, ref), "the synchronous call differs from the oracle"
    none = dict(s, kf_matched=np.zeros(len(s["k"]), np.uint8))
    ref0, nref0 = MC.oracle_run("sim3_projection", none, p)
    kf, table, d_valid = _kf_of(api, ctx, st, s, None), _Table(s), upload(s["valid"], pad=PAD)[0]
    d_matched, d_zero = upload(s["kf_matched"], pad=PAD)[0], upload(none["kf_matched"], pad=PAD)[0]
    torch.cuda.synchronize()
    for call, (d_m, r, nr) in enumerate(((d_matched, ref, nref), (d_matched, ref, nref), (None, ref0, nref0), (d_zero, ref0, nref0))):
        out = _OutProj(table.n, kf.n)
        _enqueue_proj(ctx, kf.rec, s, table, d_valid, d_m, p[0], out, st)
        st.synchronize()
        out.check(r, nr, "%s, call %d" % (what, call))
    kf.off.fetch(), kf.idx.fetch()  # the grid's guards


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", BYSIM3_INPUTS)
def test_gpu_search_by_sim3_equals_the_oracle_and_the_synchronous_call(gpu, name):
    import torch
    api, ctx, st = gpu
    s, p = MC.build(name), MC.INPUTS[name][1]["by_sim3"]
    ref, nref = MC.oracle_run("by_sim3", s, p)
    sref, snref = hip_run(ctx, "by_sim3", s, p)
    assert snref == nref and np.array_equal(sref, ref), "the synchronous call differs from the oracle"
    assert nref > 0
    pair = _Pair(api, ctx, st, s)
    torch.cuda.synchronize()
    for call in range(2):
        out = _Out12(pair.kf1.n)
        pair.enqueue(ctx, p[0], out, st)
        st.synchronize()
        out.check(ref, nref, "%s / by_sim3, call %d" % (name, call))
    for kf in (pair.kf1, pair.kf2):
        kf.off.fetch(), kf.idx.fetch()


@pytest.mark.gpu
@pytest.mark.parametrize("name", PROJ_INPUTS)
def test_gpu_search_by_projection_sim3_equals_the_oracle_and_the_synchronous_call(gpu, name):
    _run_projection(gpu, MC.build(name), MC.INPUTS[name][1]["sim3_projection"], name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CROWD_COUNTS))
def test_gpu_search_by_projection_sim3_on_a_crowd(gpu, name):
    s, p = crowd(name)
    _run_projection(gpu, s, p, "crowd of " + name)


@pytest.mark.gpu
def test_gpu_projection_through_an_index_list(gpu):
    """The table permuted and read through the index that undoes the permutation: the plain table's result.  An entry equal to n_rows
    and one equal to -1 are refused before they address the table: status, -1 for those queries, the others as if the two were invalid."""
    import torch
    api, ctx, st = gpu
    full, p = MC.build("sim3_51"), MC.INPUTS["sim3_51"][1]["sim3_projection"]
    n_rows = len(full["pos"])
    n = n_rows - 1  # one query fewer than the table has rows: the last workgroup is not full
    fields = ("pos", "normal", "max_d", "min_d", "desc")
    s = dict(full, valid=full["valid"][:n], **{key: full[key][:n] for key in fields})
    ref, nref = MC.oracle_run("sim3_projection", s, p)
    perm = np.random.default_rng(5).permutation(n_rows)
    index = np.argsort(perm).astype(np.int32)[:n]  # row index[q] of the permuted table is point q
    shuffled = dict(full, **{key: full[key][perm] for key in fields})
    assert n % 4 and nref > 100 and not np.array_equal(index, np.arange(n))
    kf, table = _kf_of(api, ctx, st, s, None), _Table(shuffled)
    d_valid, d_matched, d_index = upload(s["valid"], pad=PAD)[0], upload(s["kf_matched"], pad=PAD)[0], upload(index, pad=PAD)[0]
    out = _OutProj(n, kf.n)
    torch.cuda.synchronize()
    _enqueue_proj(ctx, kf.rec, s, table, d_valid, d_matched, p[0], out, st, n_pts=n, d_index=d_index)
    st.synchronize()
    out.check(ref, nref, "index list")
    hit = np.nonzero(ref >= 0)[0]
    bad_index = index.copy()
    bad_index[hit[0]], bad_index[hit[1]] = n_rows, -1
    without = s["valid"].copy()
    without[hit[:2]] = 0
    expect, _ = MC.oracle_run("sim3_projection", dict(s, valid=without), p)
    d_bad = upload(bad_index, pad=PAD)[0]
    out = _OutProj(n, kf.n)
    torch.cuda.synchronize()
    _enqueue_proj(ctx, kf.rec, s, table, d_valid, d_matched, p[0], out, st, n_pts=n, d_index=d_bad)
    st.synchronize()
    pt, _, _, status = out.fetch()  # and the guards
    assert status == api.ERR_INVALID and (pt[hit[:2]] == -1).all() and np.array_equal(pt, expect)


@pytest.mark.gpu
def test_gpu_degenerate_sizes(gpu):
    import torch
    api, ctx, st = gpu
    s, p = MC.build("among"), MC.INPUTS["among"][1]
    n_pts = len(s["pos"])
    kf, table, d_valid, d_matched = _kf_of(api, ctx, st, s, None), _Table(s), upload(s["valid"], pad=PAD)[0], upload(s["kf_matched"], pad=PAD)[0]
    empty = api.GridKeyframe(0, 0, 0, 0, 0, *[float(b) for b in s["bounds"]], 0, 1)  # a keyframe without keypoints: no array at all
    torch.cuda.synchronize()
    out = _OutProj(0, kf.n)  # n_pts == 0: every keypoint free, count 0, status 0, d_pt_match untouched
    _enqueue_proj(ctx, kf.rec, s, table, d_valid, d_matched, p["sim3_projection"][0], out, st, n_pts=0)
    st.synchronize()
    _, kfm, count, status = out.fetch()
    assert (kfm == -1).all() and (count, status) == (0, 0) and out.pt.untouched()
    out = _OutProj(n_pts, 0)  # kf->n == 0: every query -1, d_kf_match untouched
    _enqueue_proj(ctx, empty, s, table, d_valid, None, p["sim3_projection"][0], out, st)
    st.synchronize()
    pt, _, count, status = out.fetch()
    assert (pt == -1).all() and (count, status) == (0, 0) and out.kf.untouched()
    pair = _Pair(api, ctx, st, s)
    torch.cuda.synchronize()
    out = _Out12(0)  # kf1->n == 0: count 0, status 0, d_match12 untouched
    pair.enqueue(ctx, p["by_sim3"][0], out, st, rec1=empty, p1=[0] * 5)
    st.synchronize()
    assert out.fetch()[1:] == (0, 0) and out.match.untouched()
    out = _Out12(pair.kf1.n)  # kf2->n == 0: every entry -1
    pair.enqueue(ctx, p["by_sim3"][0], out, st, rec2=empty, p2=[0] * 5)
    st.synchronize()
    out.check(np.full(pair.kf1.n, -1, np.int32), 0, "kf2->n == 0")


@pytest.mark.gpu
def test_gpu_corrupt_records_are_reported_in_the_status(gpu):
    """A descending offset, an offset beyond n, a cell_idx entry equal to n and an octave equal to nlevels on a candidate keypoint, in
    the record both calls walk: status ORBFE_ERR_INVALID, nothing written outside the outputs, and the next clean call exact."""
    import torch
    api, ctx, st = gpu
    s, p = MC.build("among"), MC.INPUTS["among"][1]
    ref12, nref12 = MC.oracle_run("by_sim3", s, p["by_sim3"])
    refp, nrefp = MC.oracle_run("sim3_projection", s, p["sim3_projection"])
    n, n_pts = len(s["k"]), len(s["pos"])
    pair, table, d_valid, d_matched = _Pair(api, ctx, st, s), _Table(s), upload(s["valid"], pad=PAD)[0], upload(s["kf_matched"], pad=PAD)[0]
    kf = pair.kf2  # s["k"]: the keyframe the projection matcher searches and direction 1 -> 2 of SearchBySim3 walks
    st.synchronize()
    off, idx = kf.off.fetch().copy(), kf.idx.fetch().copy()

    def corrupt(cand):
        """Records that are wrong at keypoint `cand`, which the call's reference result holds: its cell is walked."""
        j = int(np.nonzero(idx[: off[CELLS]] == cand)[0][0])
        cell = int(np.searchsorted(off, j, side="right")) - 1
        assert off[cell] <= j < off[cell + 1]
        bad_octave = s["k"].copy()
        bad_octave["octave"][cand] = MC.NL
        bad_idx = idx.copy()
        bad_idx[j] = n
        descending, beyond = off.copy(), off.copy()
        descending[cell + 1] = off[cell] - 1
        beyond[cell + 1] = n + 5  # a missed check reads five guard cells of cell_idx
        keep = [upload(bad_octave, pad=PAD)[0], Guarded(bad_idx), Guarded(descending), Guarded(beyond)]
        return keep, {"octave == nlevels on a candidate keypoint": kf.record(keys=keep[0]), "a cell_idx entry equal to n": kf.record(idx=keep[1]),
                      "a descending cell_off": kf.record(off=keep[2]), "a cell_off beyond n": kf.record(off=keep[3])}

    keep12, cases12 = corrupt(int(ref12[ref12 >= 0][0]))
    keepp, casesp = corrupt(int(refp[refp >= 0][0]))
    torch.cuda.synchronize()
    for what, rec in cases12.items():
        out = _Out12(pair.kf1.n)
        pair.enqueue(ctx, p["by_sim3"][0], out, st, rec2=rec)
        st.synchronize()
        assert out.fetch()[2] == api.ERR_INVALID, ("by_sim3", what)  # and the guards
        out = _Out12(pair.kf1.n)
        pair.enqueue(ctx, p["by_sim3"][0], out, st)
        st.synchronize()
        out.check(ref12, nref12, "by_sim3, clean call after: " + what)
    for what, rec in casesp.items():
        out = _OutProj(n_pts, n)
        _enqueue_proj(ctx, rec, s, table, d_valid, d_matched, p["sim3_projection"][0], out, st)
        st.synchronize()
        assert out.fetch()[3] == api.ERR_INVALID, ("sim3_projection", what)
        out = _OutProj(n_pts, n)
        _enqueue_proj(ctx, kf.rec, s, table, d_valid, d_matched, p["sim3_projection"][0], out, st)
        st.synchronize()
        out.check(refp, nrefp, "sim3_projection, clean call after: " + what)
    # the refused grids were inputs: they and their guards are as they were uploaded
    for keep in (keep12, keepp):
        for g in keep[1:]:
            g.fetch()
    assert np.array_equal(kf.idx.fetch(), idx) and np.array_equal(kf.off.fetch(), off)
    # what the host can see is refused by the call itself and queues nothing
    out, out12 = _OutProj(n_pts, n), _Out12(pair.kf1.n)
    null_keys = kf.record()
    null_keys.keys_un = None
    descending_bounds = kf.record()
    descending_bounds.max_x = descending_bounds.min_x
    for rec in (null_keys, kf.record(n=65536), kf.record(n=-1), descending_bounds):
        with pytest.raises(api.OrbfeError):
            _enqueue_proj(ctx, rec, s, table, d_valid, d_matched, 4.0, out, st)
        with pytest.raises(api.OrbfeError):
            pair.enqueue(ctx, 4.0, out12, st, rec2=rec)
    with pytest.raises(api.OrbfeError):  # more queries than rows without an index list
        _enqueue_proj(ctx, kf.rec, s, table, d_valid, d_matched, 4.0, out, st, n_pts=table.n + 1)
    with pytest.raises(api.OrbfeError):
        _enqueue_proj(ctx, kf.rec, s, table, d_valid, d_matched, 4.0, out, st, n_pts=-1)
    with pytest.raises(api.OrbfeError):  # a NULL output
        ctx.enqueue_search_by_projection_sim3(kf.rec, s["Scw"], table.n, 0, table.n, *table.ptrs(), d_valid.data_ptr(), 0, 4.0, out.ptrs()[0], 0,
                                              out.ptrs()[2], out.ptrs()[3], stream=st.cuda_stream)
    st.synchronize()
    assert all(g.untouched() for g in (out.pt, out.kf, out.count, out.status, out12.match, out12.count, out12.status))


@pytest.mark.gpu
def test_gpu_compute_sim3_sequence_on_one_stream(gpu):
    """SearchBySim3, then -- without a host step -- the keypoints it matched become d_kf_matched of SearchByProjection on the first
    keyframe (a torch op on the stream), then a second, different SearchBySim3 that reuses the scratch.  One synchronise at the end."""
    import torch
    api, ctx, st = gpu
    a, pa = MC.build("among"), MC.INPUTS["among"][1]
    b, pb = MC.build("sideways"), MC.INPUTS["sideways"][1]
    assert len(a["k1"]) != len(b["k1"]) and len(a["k"]) != len(b["k"])
    ref_a = MC.oracle_run("by_sim3", a, pa["by_sim3"])
    ref_b = MC.oracle_run("by_sim3", b, pb["by_sim3"])
    # the projection call searches the FIRST keyframe of `a` (camera at the origin) for the map points of the scene
    Scw = a["T_last"].copy(); Scw *= np.float32(1.07)
    proj = dict(a, k=a["k1"], d=a["d1"], Scw=Scw, kf_matched=(ref_a[0] >= 0).astype(np.uint8))
    ref_p = MC.oracle_run("sim3_projection", proj, pa["sim3_projection"])
    free = MC.oracle_run("sim3_projection", dict(proj, kf_matched=np.zeros(len(a["k1"]), np.uint8)), pa["sim3_projection"])
    assert ref_a[1] > 20 and ref_b[1] > 20 and ref_p[1] > 20 and not np.array_equal(ref_p[0], free[0])
    pair_a, pair_b = _Pair(api, ctx, st, a), _Pair(api, ctx, st, b)
    table, d_valid = _Table(a), upload(a["valid"], pad=PAD)[0]
    n1 = pair_a.kf1.n
    out_a, out_p, out_b = _Out12(n1), _OutProj(table.n, n1), _Out12(pair_b.kf1.n)
    d_matched = torch.zeros(n1 + 64, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        pair_a.enqueue(ctx, pa["by_sim3"][0], out_a, st)
        d_matched[:n1] = (out_a.match.view >= 0).to(torch.uint8)
        _enqueue_proj(ctx, pair_a.kf1.rec, proj, table, d_valid, d_matched, pa["sim3_projection"][0], out_p, st)
        pair_b.enqueue(ctx, pb["by_sim3"][0], out_b, st)
    st.synchronize()
    out_a.check(ref_a[0], ref_a[1], "first SearchBySim3")
    out_p.check(ref_p[0], ref_p[1], "SearchByProjection behind it")
    out_b.check(ref_b[0], ref_b[1], "second SearchBySim3")
