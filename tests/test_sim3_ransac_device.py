"""orbfe_enqueue_sim3_ransac_batch / orbfe_enqueue_sim3_ransac_select / orbfe_sim3_ransac (Sim3Solver, reference src/Sim3Solver.cc;
orbslam2_amd/csrc/orbfe_sim3_ransac.hip) against the model (tests/sim3_solver_model.py) on the scenes of tests/sim3_solver_scenes.py, which
tests/test_sim3_solver_model.py has checked on the CPU.  The arithmetic is fully stated, so everything is compared
EXACTLY and nothing is left out: counts, d_corr, the sets, the bits of every d_hyp record, the inlier bit rows, the events, the status.

Shapes are the smallest that reach each path: 96 and 80 keypoint slots with 40 pairs and max_its 300 (clean, outliers), max_its 12
elsewhere; 64, 65 and 70 correspondences (the word boundary and the tail bits); one scene of ORBFE_SIM3_RANSAC_LDS_SLOTS + 1
correspondences for the table in HBM.  Device arrays and guards follow tests/device_arrays.py: inputs between PAD readable entries,
outputs between sentinel rows, never the default stream."""
import numpy as np
import pytest

from tests import sim3_solver_model as M
from tests import sim3_solver_scenes as S
from tests.device_arrays import Guarded, context, upload, upload_records

PAD = 64
FILL = 0x5B                    # what every output byte holds before a call: no row of the model is made of it
ROWS = ("status", "n_corr", "n_its", "n_events", "corr", "sets", "hyp", "bits", "events")


@pytest.fixture(scope="module")
def gpu():
    import torch
    from orbslam2_amd import api
    ctx = context(api)
    assert np.array_equal(ctx.tables()["sigma2"][:S.NLEVELS], S.SIGMA2)
    assert api.SIM3_RANSAC_LDS_SLOTS == S.LDS_SLOTS
    yield api, ctx, torch.cuda.Stream()
    ctx.close()


def _up(own, a):
    t, p = upload(a, front=PAD, pad=PAD)
    own.append(t)
    return p


def _filled(shape, dtype):
    a = np.empty(shape, dtype)
    a.view(np.uint8).reshape(-1)[:] = FILL
    return a


class _Batch:
    """KF1 and the candidates of a list of scenes (which share KF1 and the call's parameters) in HBM, fresh guarded outputs.  rec_n:
    {candidate: the record's n}, to lie about a keyframe's size."""

    def __init__(self, api, scenes, rec_n=None, with_sets=True):
        s0 = scenes[0]
        self.s0, self.n, self.own = s0, len(scenes), []
        self.max_pairs, self.max_its, self.max_kf_n = s0["max_pairs"], s0["max_its"], s0["max_kf_n"]
        self.words = (self.max_pairs + 31) // 32
        self.kf1 = api.GridKeyframe()
        self.kf1.keys_un, self.kf1.n = _up(self.own, s0["keys1"]), len(s0["keys1"])
        self.pos1, self.valid1 = _up(self.own, s0["pos1"]), _up(self.own, s0["valid1"].astype(np.int32))
        self.table = _up(self.own, s0["its_for_n"])
        recs = []
        for c, s in enumerate(scenes):
            assert s["keys1"] is s0["keys1"] and np.array_equal(s["valid1"], s0["valid1"]) and s["max_pairs"] == self.max_pairs and s["max_its"] == self.max_its
            r = api.Sim3RansacCandidate()
            r.keys_un, r.pos, r.valid = _up(self.own, s["keys2"]), _up(self.own, s["pos2"]), _up(self.own, s["valid2"].astype(np.int32))
            r.T2w = _up(self.own, s["T2w"].reshape(-1))
            rows = np.full((self.max_pairs, 2), 0, np.int32)           # the whole row of d_pairs is readable; the count says how much counts
            rows[:len(s["pairs"])] = s["pairs"]
            r.pairs, r.n_pairs = _up(self.own, rows), _up(self.own, np.array([len(s["pairs"])], np.int32))
            r.draws = _up(self.own, np.ascontiguousarray(s["draws"], np.uint32).view(np.int32))
            r.n = (rec_n or {}).get(c, len(s["keys2"]))
            recs.append(r)
        self.recs = upload_records(recs)
        n, mi, mp = self.n, self.max_its, self.max_pairs
        self.out = dict(n_corr=Guarded(_filled(n, np.int32)), n_its=Guarded(_filled(n, np.int32)), corr=Guarded(_filled((n * mp, 2), np.int32)),
                        sets=Guarded(_filled((n * mi, 3), np.int32)) if with_sets else None, hyp=Guarded(_filled(n * mi, M.HYP_DTYPE)),
                        bits=Guarded(_filled((n * mi, self.words), np.uint32)), events=Guarded(_filled(n * mi, np.int32)),
                        n_events=Guarded(_filled(n, np.int32)), status=Guarded(_filled(n, np.int32)))

    def args(self, **kw):
        o = self.out
        a = dict(kf1=self.kf1, T1w=self.s0["T1w"], pos1=self.pos1, valid1=self.valid1, cands=self.recs.data_ptr(), n_cands=self.n, max_pairs=self.max_pairs,
                 max_kf_n=self.max_kf_n, fix_scale=self.s0["fix_scale"], min_inliers=self.s0["min_inliers"], max_its=self.max_its, table=self.table,
                 **{k: (g.ptr if g is not None else 0) for k, g in o.items()})
        a.update(kw)
        return a

    def enqueue(self, ctx, st, **kw):
        a = self.args(**kw)
        ctx.enqueue_sim3_ransac_batch(a["kf1"], a["T1w"], a["pos1"], a["valid1"], a["cands"], a["n_cands"], a["max_pairs"], a["max_kf_n"], a["fix_scale"],
                                      a["min_inliers"], a["max_its"], a["table"], a["n_corr"], a["n_its"], a["corr"], a["sets"], a["hyp"], a["bits"], a["events"],
                                      a["n_events"], a["status"], stream=st.cuda_stream)

    def untouched(self):
        return all(g.untouched() for g in self.out.values() if g is not None)

    def fetch(self):
        """One dict per candidate, shaped as the model's."""
        f = {k: g.fetch() for k, g in self.out.items() if g is not None}
        mi, mp = self.max_its, self.max_pairs
        rows = []
        for c in range(self.n):
            r = dict(status=int(f["status"][c]), n_corr=int(f["n_corr"][c]), n_its=int(f["n_its"][c]), n_events=int(f["n_events"][c]),
                     corr=f["corr"][c * mp:(c + 1) * mp], hyp=f["hyp"][c * mi:(c + 1) * mi], bits=f["bits"][c * mi:(c + 1) * mi], events=f["events"][c * mi:(c + 1) * mi])
            if "sets" in f:
                r["sets"] = f["sets"][c * mi:(c + 1) * mi]
            rows.append(r)
        return rows


def _assert_same(got, ref, what):
    for k in ROWS:
        if k not in got:
            continue
        if k == "hyp":
            assert np.array_equal(got[k]["n_inliers"], ref[k]["n_inliers"]), (what, "counts", got[k]["n_inliers"][:12], ref[k]["n_inliers"][:12])
            bad = np.nonzero((got[k].view(np.uint32).reshape(-1, 16) != ref[k].view(np.uint32).reshape(-1, 16)).any(1))[0]
            assert bad.size == 0, (what, "hypothesis records differ at", bad[:8].tolist(), got[k][bad[:1]], ref[k][bad[:1]])
        elif isinstance(ref[k], np.ndarray):
            assert np.array_equal(got[k], ref[k]), (what, k, np.argwhere(got[k] != ref[k])[:8].tolist())
        else:
            assert got[k] == ref[k], (what, k, got[k], ref[k])


def _alone(gpu, s, **kw):
    api, ctx, st = gpu
    b = _Batch(api, [s], **kw)
    b.enqueue(ctx, st)
    st.synchronize()
    return b.fetch()[0]


@pytest.mark.gpu
@pytest.mark.parametrize("name", S.DEVICE_SCENES)
def test_gpu_scene_equals_the_model_bit_for_bit(gpu, name):
    """clean / outliers: 300 hypotheses; fix_scale; n64 n65 n70: the word boundary and the tail bits; hbm: the table read from HBM;
    invalid_slots: N < n_pairs, d_corr skips them; below_min: no iteration, no event; at_min: one iteration; gate: the truncated
    gates; coincident: den == 0."""
    got, ref = _alone(gpu, S.scene(name)), S.model(name)
    print("%-14s N %4d iterations %3d events %3d best count %d" % (name, got["n_corr"], got["n_its"], got["n_events"], got["hyp"]["n_inliers"].max()))
    _assert_same(got, ref, name)
    if name == "gate":
        K, J = S.gate_case()[:2]
        assert not (got["bits"][K][J >> 5] >> np.uint32(J & 31)) & 1 and got["hyp"]["n_inliers"][K] == got["n_corr"] - 1
    if name == "coincident":
        h = got["hyp"][0]
        assert h["n_inliers"] == 0 and np.array_equal(h["R12"], np.eye(3, dtype=np.float32).reshape(9)) and h["s12"].view(np.uint32) == M.NAN_BITS
    if name == "below_min":
        assert got["n_its"] == 0 and got["n_events"] == 0 and (got["events"] == -1).all() and not got["hyp"].view(np.uint8).any()
    if name == "at_min":
        assert got["n_its"] == 1
    if name in ("n65", "n70"):
        N = got["n_corr"]
        assert not (got["bits"][:, N >> 5] >> np.uint32(N & 31)).any()       # tail bits are 0


def _bad_pair(s, k, pair):
    b = dict(s, pairs=s["pairs"].copy())
    b["pairs"][k] = pair
    return b


@pytest.mark.gpu
def test_gpu_batch_with_bad_records_equals_each_candidate_alone(gpu):
    """Three launches for any number of candidates; a record the device refuses (n > max_kf_n) or a pair index out of range reports
    ORBFE_ERR_INVALID in its own row and changes no other row."""
    api, ctx, st = gpu
    a, b = S.scene("cand_a"), S.scene("cand_b")
    a = dict(a, max_pairs=b["max_pairs"])                              # one call: one max_pairs, one table
    a["its_for_n"] = b["its_for_n"]
    assert np.array_equal(M.its_table(40, S.PROB, S.MIN_INLIERS, 12), b["its_for_n"])
    high, neg = _bad_pair(a, 5, (a["pairs"][5, 0], len(a["keys2"]))), _bad_pair(a, 7, (-1, a["pairs"][7, 1]))
    scenes = [a, high, b, a, neg]
    batch = _Batch(api, scenes, rec_n={3: a["max_kf_n"] + 1})
    batch.enqueue(ctx, st)
    st.synchronize()
    got = batch.fetch()
    refs = [M.run(s) for s in scenes]
    refs[3] = M.run(dict(a, keys2=np.zeros(a["max_kf_n"] + 1, S.KP_DTYPE)))
    for c, (g, r) in enumerate(zip(got, refs)):
        _assert_same(g, r, "candidate %d" % c)
    assert [g["status"] for g in got] == [0, M.ERR_INVALID, 0, M.ERR_INVALID, M.ERR_INVALID]
    assert got[1]["n_corr"] == got[0]["n_corr"] - 1 and got[3]["n_corr"] == 0 and got[3]["n_its"] == 0
    for c in (0, 2):
        _assert_same(got[c], _alone(gpu, scenes[c]), "candidate %d alone" % c)
    again = _Batch(api, scenes, rec_n={3: a["max_kf_n"] + 1})          # and run to run
    again.enqueue(ctx, st)
    st.synchronize()
    for g, h in zip(got, again.fetch()):
        _assert_same(g, h, "second run")


@pytest.mark.gpu
def test_gpu_sets_are_optional_and_calls_queued_on_one_stream_equal_each_alone(gpu):
    api, ctx, st = gpu
    names = ["hbm", "outliers", "n65", "hbm"]                          # the scratch grows and is reused between calls without a host wait
    calls = [_Batch(api, [S.scene(n)], with_sets=(i != 1)) for i, n in enumerate(names)]
    for c in calls:
        c.enqueue(ctx, st)
    st.synchronize()
    for n, c in zip(names, calls):
        _assert_same(c.fetch()[0], S.model(n), n)


@pytest.mark.gpu
def test_gpu_synchronous_form_equals_the_enqueue_form(gpu):
    api, ctx, st = gpu
    for name in ("outliers", "n70", "invalid_slots", "below_min", "coincident"):
        s = S.scene(name)
        got = ctx.sim3_ransac(s["keys1"], s["T1w"], s["pos1"], s["valid1"], s["keys2"], s["T2w"], s["pos2"], s["valid2"], s["pairs"], s["draws"], s["fix_scale"],
                              s["min_inliers"], s["max_its"], s["its_for_n"])
        _assert_same(got, _alone(gpu, s), name)
    s = S.scene("below_min")                                           # no keypoint on either side and n_pairs = 0: every padded array of the call is empty
    s = dict(s, **{k: s[k][:0] for k in ("keys1", "pos1", "valid1", "keys2", "pos2", "valid2", "pairs")}, max_pairs=1, max_kf_n=0)
    got = ctx.sim3_ransac(s["keys1"], s["T1w"], s["pos1"], s["valid1"], s["keys2"], s["T2w"], s["pos2"], s["valid2"], s["pairs"], s["draws"], s["fix_scale"],
                          s["min_inliers"], s["max_its"], s["its_for_n"])
    _assert_same(got, M.run(s), "empty")
    assert got["n_corr"] == 0 and got["n_its"] == 0 and got["n_events"] == 0 and (got["corr"] == -1).all()
    s = _bad_pair(S.scene("cand_a"), 5, (0, 4000))                     # what only the device sees comes back as the call's error
    with pytest.raises(api.OrbfeError) as e:
        ctx.sim3_ransac(s["keys1"], s["T1w"], s["pos1"], s["valid1"], s["keys2"], s["T2w"], s["pos2"], s["valid2"], s["pairs"], s["draws"], 0, 20, 12, s["its_for_n"])
    assert e.value.code == api.ERR_INVALID
    assert np.array_equal(api.sim3_iteration_table(400), M.its_table(400, 0.99, 20, 300))


@pytest.mark.gpu
def test_gpu_bad_arguments_are_refused_and_queue_nothing(gpu):
    api, ctx, st = gpu
    b = _Batch(api, [S.scene("cand_a")])
    big = api.GridKeyframe(); big.keys_un, big.n = b.kf1.keys_un, b.max_kf_n + 1
    neg = api.GridKeyframe(); neg.keys_un, neg.n = b.kf1.keys_un, -1
    nokeys = api.GridKeyframe(); nokeys.n = b.kf1.n
    for kw in (dict(kf1=None), dict(kf1=big), dict(kf1=neg), dict(kf1=nokeys), dict(pos1=0), dict(valid1=0), dict(cands=0), dict(table=0), dict(n_cands=-1),
               dict(n_cands=65536), dict(max_pairs=0), dict(max_pairs=-3), dict(max_kf_n=-1), dict(max_kf_n=65536), dict(min_inliers=2), dict(max_its=0),
               dict(max_its=-1), dict(n_corr=0), dict(n_its=0), dict(corr=0), dict(hyp=0), dict(bits=0), dict(events=0), dict(n_events=0), dict(status=0)):
        with pytest.raises(api.OrbfeError) as e:
            b.enqueue(ctx, st, **kw)
        assert e.value.code == api.ERR_INVALID, kw
    b.enqueue(ctx, st, n_cands=0)                                       # ORBFE_OK, nothing queued
    st.synchronize()
    assert b.untouched()


class _Select:
    def __init__(self, n1, max_kf_n):
        self.prior, self.v1, self.v2, self.status = Guarded.cells(n1), Guarded.cells(n1), Guarded.cells(max_kf_n), Guarded.cells(1)

    def enqueue(self, ctx, st, b, c, k, **kw):
        a = dict(cands=b.recs.data_ptr(), n_cands=b.n, c=c, k=k, n1=b.kf1.n, valid1=b.valid1, max_pairs=b.max_pairs, max_kf_n=b.max_kf_n, max_its=b.max_its)
        a.update(kw)
        o = b.out
        ctx.enqueue_sim3_ransac_select(a["cands"], a["n_cands"], a["c"], a["k"], a["n1"], a["valid1"], a["max_pairs"], a["max_kf_n"], a["max_its"], o["n_corr"].ptr,
                                       o["n_its"].ptr, o["corr"].ptr, o["bits"].ptr, self.prior.ptr, self.v1.ptr, self.v2.ptr, self.status.ptr, stream=st.cuda_stream)

    def fetch(self):
        return self.prior.fetch(), self.v1.fetch(), self.v2.fetch(), int(self.status.fetch()[0])


@pytest.mark.gpu
def test_gpu_select_rows_equal_the_model(gpu):
    api, ctx, st = gpu
    a, b = S.scene("cand_a"), S.scene("cand_b")
    a = dict(a, max_pairs=b["max_pairs"], its_for_n=b["its_for_n"])
    scenes = [a, b]
    batch = _Batch(api, scenes)
    batch.enqueue(ctx, st)                                              # no host wait between the calls
    picks = [(0, 1), (1, 3), (0, 11), (1, 0)]
    sels = [_Select(batch.kf1.n, batch.max_kf_n) for _ in picks]
    for sel, (c, k) in zip(sels, picks):
        sel.enqueue(ctx, st, batch, c, k)
    st.synchronize()
    rows = batch.fetch()
    for sel, (c, k) in zip(sels, picks):
        s = scenes[c]
        prior, v1, v2, status = sel.fetch()
        rp, r1, r2 = M.select_rows(rows[c], k, len(s["keys1"]), s["valid1"], s["valid2"])
        n2 = len(s["keys2"])
        assert status == 0 and np.array_equal(prior, rp) and np.array_equal(v1, r1) and np.array_equal(v2[:n2], r2), (c, k)
        assert (v2[n2:] == -7).all()                                    # the entries beyond the record's n are left untouched
        assert (prior >= 0).sum() == rows[c]["hyp"]["n_inliers"][k] and ((s["valid2"] != 0).sum() - v2[:n2].sum()) == (prior >= 0).sum()
    assert max(rows[c]["hyp"]["n_inliers"][k] for c, k in picks) > 20   # the rows decide something
    late = _Select(batch.kf1.n, batch.max_kf_n)                         # k beyond the candidate's iterations: the status, nothing selected
    small = _Batch(api, [S.scene("at_min")])
    small.enqueue(ctx, st)
    late.enqueue(ctx, st, small, 0, 5)
    st.synchronize()
    prior, v1, v2, status = late.fetch()
    s = S.scene("at_min")
    assert status == M.ERR_INVALID and (prior == -1).all() and np.array_equal(v1, (s["valid1"] != 0).astype(np.int32))
    fresh = _Select(batch.kf1.n, batch.max_kf_n)
    for kw in (dict(c=-1), dict(c=2), dict(k=-1), dict(k=12), dict(cands=0), dict(valid1=0), dict(n1=-1), dict(max_pairs=0), dict(max_kf_n=65536)):
        with pytest.raises(api.OrbfeError) as e:
            fresh.enqueue(ctx, st, batch, kw.pop("c", 0), kw.pop("k", 0), **kw)
        assert e.value.code == api.ERR_INVALID, kw
    st.synchronize()
    assert all(g.untouched() for g in (fresh.prior, fresh.v1, fresh.v2, fresh.status))


@pytest.mark.gpu
def test_gpu_round_without_uploads_equals_the_per_call_path(gpu):
    """ransac -> (one download of the events and d_hyp) -> select -> SearchBySim3 -> OptimizeSim3 on one stream against the existing path:
    the same two calls fed by host uploads of d_prior12 and the two valid arrays that the model forms from the fetched rows.  match12, S12
    and the counts are bit-equal, and two runs give the same bits."""
    from tests import matcher_census as MC
    from tests.test_sim3_device import _Out12, _Pair
    api, ctx, st = gpu
    a, th = MC.build("among"), MC.INPUTS["among"][1]["by_sim3"][0]
    ref = MC.oracle_run("by_sim3", a, MC.INPUTS["among"][1]["by_sim3"])
    n1, n2 = len(a["k1"]), len(a["k"])
    idx1 = np.nonzero(ref[0] >= 0)[0][:40]
    assert len(idx1) > 20                                              # more than min_inliers pairs: the solver iterates
    pos1, pos2 = np.ascontiguousarray(a["pts1"][0], np.float32).reshape(n1, 3), np.ascontiguousarray(a["pts2"][0], np.float32).reshape(n2, 3)
    valid1, valid2 = np.asarray(a["pts1"][4], np.int32).copy(), np.asarray(a["pts2"][4], np.int32).copy()
    valid1[idx1], valid2[ref[0][idx1]] = 1, 1
    s = dict(keys1=np.ascontiguousarray(a["k1"]), pos1=pos1, valid1=valid1, T1w=np.ascontiguousarray(a["T_last"], np.float32)[:3], keys2=np.ascontiguousarray(a["k"]),
             pos2=pos2, valid2=valid2, T2w=np.ascontiguousarray(a["T_cur"], np.float32)[:3], pairs=np.stack([idx1, ref[0][idx1]], 1).astype(np.int32),
             draws=S.draws(77, 12), fix_scale=0, min_inliers=20, max_its=12, max_pairs=len(idx1), max_kf_n=max(n1, n2),
             its_for_n=M.its_table(len(idx1), S.PROB, 20, 12))
    pair = _Pair(api, ctx, st, a)
    pts = lambda side, d_valid: [t.data_ptr() for t in (pair.p1 if side == 1 else pair.p2)[:4]] + [d_valid]
    own = []
    d_pos1, d_pos2, d_valid1, d_valid2 = _up(own, pos1), _up(own, pos2), _up(own, valid1), _up(own, valid2)

    def round_(prior, v1, v2, hyp):
        out, S12, n_in, status = _Out12(n1), Guarded(np.full(8, np.nan)), Guarded.cells(1), Guarded.cells(1)
        ctx.enqueue_search_by_sim3(pair.kf1.rec, s["T1w"], pts(1, v1), pair.kf2.rec, s["T2w"], pts(2, v2), hyp["s12"], hyp["R12"], hyp["t12"], th, *out.ptrs(),
                                   stream=st.cuda_stream)
        ctx.enqueue_optimize_sim3(pair.kf1.rec, s["T1w"], d_pos1, d_valid1, pair.kf2.rec, s["T2w"], d_pos2, d_valid2, hyp["s12"], hyp["R12"], hyp["t12"], 10.0, 0,
                                  out.match.ptr, S12.ptr, n_in.ptr, status.ptr, d_prior12=prior, stream=st.cuda_stream)
        return out, S12, n_in, status

    def device_path():
        batch = _Batch(api, [s])
        batch.enqueue(ctx, st)
        st.synchronize()                                                # the one download: events and d_hyp
        rows = batch.fetch()[0]
        k = int(rows["events"][0]) if rows["n_events"] else 0
        sel = _Select(n1, batch.max_kf_n)
        sel.enqueue(ctx, st, batch, 0, k)
        res = round_(sel.prior.ptr, sel.v1.ptr, sel.v2.ptr, rows["hyp"][k])
        st.synchronize()
        return rows, k, [g.fetch() for g in (res[0].match, res[0].count, res[1], res[2], res[3])], (batch, sel)

    rows, k, dev, _ = device_path()
    assert rows["status"] == 0 and rows["n_corr"] == len(idx1) and rows["n_its"] == s["its_for_n"][len(idx1)] > 1
    prior, v1, v2 = M.select_rows(rows, k, n1, valid1, valid2)
    res = round_(_up(own, prior), _up(own, v1), _up(own, v2), rows["hyp"][k])
    st.synchronize()
    host = [g.fetch() for g in (res[0].match, res[0].count, res[1], res[2], res[3])]
    print("round of iteration %d: %d RANSAC inliers, SearchBySim3 found %d, OptimizeSim3 kept %d" % (k, rows["hyp"]["n_inliers"][k], dev[1][0], dev[3][0]))
    for d, h in zip(dev, host):
        assert d.tobytes() == h.tobytes()
    rows2, k2, dev2, _ = device_path()
    _assert_same(rows2, rows, "second run")
    assert k2 == k and all(d.tobytes() == e.tobytes() for d, e in zip(dev, dev2))
