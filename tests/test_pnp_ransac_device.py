"""orbfe_enqueue_pnp_ransac_batch / orbfe_enqueue_pnp_ransac_select / orbfe_pnp_ransac (PnPsolver, reference src/PnPsolver.cc;
orbslam2_amd/csrc/orbfe_pnp_ransac.hip) against the model (tests/pnp_solver_model.py) on the scenes of tests/pnp_solver_scenes.py, which
tests/test_pnp_solver_model.py has checked on the CPU.  The arithmetic is fully stated, so everything is compared
EXACTLY and nothing is left out: counts, d_corr, the sets, the bits of every d_hyp and d_refined record, both inlier bit rows, the
events, the exhausted exit, the status.

The frame is image slot 0 of a real extraction call whose keypoints are then replaced by the scene's (as tests/test_matchers_device.py
does), so the rows have the context's capacity: a scene's model, made for its own keypoint count, must equal the head of every row and
the rest must be the fill the contract states.  Shapes are the smallest that reach each path: 96 keypoints against 80 keyframe slots
with 40 matches and max_its 300 (clean, outliers), 12 to 40 elsewhere; 64, 65 and 70 correspondences (the word boundary and the tail
bits); N = 4, N at and below mRansacMinInliers; one scene of ORBFE_PNP_RANSAC_LDS_SLOTS + 1 correspondences for the table in HBM.
Device arrays and guards follow tests/device_arrays.py: inputs between PAD readable entries, outputs between sentinel rows, never the
default stream."""
import numpy as np
import pytest

from tests import pnp_solver_model as M
from tests import pnp_solver_scenes as S
from tests.device_arrays import HAS_UNTOUCHED, UNTOUCHED, Guarded, context, device_buffers, upload, upload_records

PAD = 64
FILL = 0x5B                    # what every output byte holds before a call: no row of the model is made of it
ROWS = ("status", "n_corr", "n_its", "n_events", "exhausted", "corr", "sets", "hyp", "bits", "refined", "refined_bits", "events")
_tables = {}


@pytest.fixture(scope="module")
def gpu():
    import torch
    from orbslam2_amd import api
    ctx = context(api)
    assert np.array_equal(ctx.tables()["sigma2"][:S.NLEVELS], S.SIGMA2)
    assert api.PNP_RANSAC_LDS_SLOTS == S.LDS_SLOTS and ctx.capacity > S.LDS_SLOTS + 76
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


def _table(cap, s):
    key = (cap, s["min_inliers"], s["epsilon"])
    if key not in _tables:
        _tables[key] = M.its_table(cap, S.PROB, s["min_inliers"], S.MAX_ITS, s["epsilon"])
    assert np.array_equal(_tables[key][:len(s["its_for_n"])], s["its_for_n"])
    return _tables[key]


def _set_frame(ctx, keys):
    """Makes `keys` image slot 0 of a fresh extraction call (monocular keypoints: no descriptor and no mvuRight is read)."""
    from tests.test_matchers_device import _inject
    _inject(ctx, keys, np.zeros((len(keys), 32), np.uint8), np.full(len(keys), -1, np.float32))


class _Batch:
    """The candidates of a list of scenes (which share the frame and the call's parameters) in HBM, fresh guarded outputs.  rec_n:
    {candidate: the record's n}, to lie about a keyframe's size.  The frame must be slot 0 already."""

    def __init__(self, api, ctx, scenes, rec_n=None, with_sets=True):
        s0 = scenes[0]
        self.s0, self.n, self.own, self.cap = s0, len(scenes), [], ctx.capacity
        self.max_its, self.max_kf_n = s0["max_its"], max(s["max_kf_n"] for s in scenes)
        self.words = (self.cap + 31) // 32
        self.table = _up(self.own, _table(self.cap, s0))
        recs = []
        for c, s in enumerate(scenes):
            assert s["keys"] is s0["keys"] and all(s[k] == s0[k] for k in ("max_its", "min_inliers", "epsilon", "n_iterations", "th2"))
            r = api.PnPCandidate()
            row = np.full(self.cap, -1, np.int32)                      # the whole row of d_f_match is readable; the slot's count says how much counts
            row[:len(s["f_match"])] = s["f_match"]
            r.f_match, r.pos, r.valid = _up(self.own, row), _up(self.own, s["pos"]), _up(self.own, s["valid"].astype(np.int32))
            r.draws = _up(self.own, np.ascontiguousarray(s["draws"], np.uint32).view(np.int32))
            r.n = (rec_n or {}).get(c, len(s["valid"]))
            recs.append(r)
        self.recs = upload_records(recs)
        n, mi, cap, w = self.n, self.max_its, self.cap, self.words
        self.out = dict(n_corr=Guarded(_filled(n, np.int32)), n_its=Guarded(_filled(n, np.int32)), corr=Guarded(_filled((n * cap, 2), np.int32)),
                        sets=Guarded(_filled((n * mi, 4), np.int32)) if with_sets else None, hyp=Guarded(_filled(n * mi, M.HYP_DTYPE)),
                        bits=Guarded(_filled((n * mi, w), np.uint32)), refined=Guarded(_filled(n * mi, M.REFINED_DTYPE)),
                        refined_bits=Guarded(_filled((n * mi, w), np.uint32)), events=Guarded(_filled(n * mi, np.int32)),
                        n_events=Guarded(_filled(n, np.int32)), exhausted=Guarded(_filled(n, np.int32)), status=Guarded(_filled(n, np.int32)))

    def args(self, **kw):
        s0 = self.s0
        a = dict(slot=0, cands=self.recs.data_ptr(), n_cands=self.n, max_kf_n=self.max_kf_n, min_inliers=s0["min_inliers"], max_its=self.max_its,
                 n_iterations=s0["n_iterations"], epsilon=s0["epsilon"], th2=s0["th2"], table=self.table, min_set=4,
                 **{k: (g.ptr if g is not None else 0) for k, g in self.out.items()})
        a.update(kw)
        return a

    def enqueue(self, ctx, st, **kw):
        a = self.args(**kw)
        ctx.enqueue_pnp_ransac_batch(a["slot"], a["cands"], a["n_cands"], a["max_kf_n"], a["min_inliers"], a["max_its"], a["n_iterations"], a["epsilon"], a["th2"],
                                     a["table"], a["n_corr"], a["n_its"], a["corr"], a["sets"], a["hyp"], a["bits"], a["refined"], a["refined_bits"], a["events"],
                                     a["n_events"], a["exhausted"], a["status"], min_set=a["min_set"], stream=st.cuda_stream)

    def untouched(self):
        return all(g.untouched() for g in self.out.values() if g is not None)

    def fetch(self):
        """One dict per candidate, shaped as the device's rows (capacity the context's)."""
        f = {k: g.fetch() for k, g in self.out.items() if g is not None}
        mi, cap = self.max_its, self.cap
        rows = []
        for c in range(self.n):
            r = {k: int(f[k][c]) for k in ("status", "n_corr", "n_its", "n_events", "exhausted")}
            r.update(corr=f["corr"][c * cap:(c + 1) * cap], **{k: f[k][c * mi:(c + 1) * mi] for k in ("hyp", "bits", "refined", "refined_bits", "events")})
            if "sets" in f:
                r["sets"] = f["sets"][c * mi:(c + 1) * mi]
            rows.append(r)
        return rows


def _crop(got, cap):
    """Device rows (the context's capacity) as rows of capacity `cap`, after checking the fill beyond it: (-1, -1) and zero words."""
    words = (cap + 31) // 32
    out = dict(got)
    assert (got["corr"][cap:] == -1).all()
    out["corr"] = got["corr"][:cap]
    for k in ("bits", "refined_bits"):
        assert not got[k][:, words:].any(), k
        out[k] = got[k][:, :words]
    return out


def _assert_same(got, ref, what):
    for k in ROWS:
        if k not in got:
            continue
        if k in ("hyp", "refined"):
            assert np.array_equal(got[k]["n_inliers"], ref[k]["n_inliers"]), (what, k, "counts", got[k]["n_inliers"][:12], ref[k]["n_inliers"][:12])
            bad = np.nonzero((got[k].view(np.uint32).reshape(-1, 16) != ref[k].view(np.uint32).reshape(-1, 16)).any(1))[0]
            assert bad.size == 0, (what, k, "records differ at", bad[:8].tolist(), got[k][bad[:1]], ref[k][bad[:1]])
        elif isinstance(ref[k], np.ndarray):
            assert got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), (what, k, np.argwhere(got[k] != ref[k])[:8].tolist())
        else:
            assert got[k] == ref[k], (what, k, got[k], ref[k])


def _alone(gpu, s, **kw):
    api, ctx, st = gpu
    _set_frame(ctx, s["keys"])
    b = _Batch(api, ctx, [s], **kw)
    b.enqueue(ctx, st)
    st.synchronize()
    return b.fetch()[0]


@pytest.mark.gpu
@pytest.mark.parametrize("name", S.DEVICE_SCENES)
def test_gpu_scene_equals_the_model_bit_for_bit(gpu, name):
    """clean / outliers: 300 hypotheses; n64 n65 n70: the word boundary and the tail bits; hbm: the table read from HBM; invalid_points:
    N below the matches; noisy: 60 hypotheses at a pixel of noise; n4, at_min: N == mRansacMinInliers, the table's 1 iteration against iterate(5)'s 5; below_min: no iteration;
    degenerate: a coincident and a coplanar draw, NaN records; last_record: the only record on the last iteration; many_records."""
    s = S.scene(name)
    got, ref = _crop(_alone(gpu, s), s["capacity"]), S.model(name)
    print("%-14s N %4d iterations %3d events %3d records %s best count %d" % (name, got["n_corr"], got["n_its"], got["n_events"], S.records(got), got["hyp"]["n_inliers"].max()))
    _assert_same(got, ref, name)
    if name == "degenerate":
        assert (got["hyp"]["Rcw"][:2].view(np.uint32) == M.NAN_BITS).all() and got["n_events"] > 0
    if name == "below_min":
        assert got["n_its"] == 0 and got["n_events"] == 0 and got["exhausted"] == -1 and (got["events"] == -1).all() and not got["hyp"]["n_inliers"].any()
    if name in ("at_min", "n4"):
        assert got["n_its"] == 5 and s["its_for_n"][got["n_corr"]] == 1
    if name == "hbm":
        assert got["n_corr"] == S.LDS_SLOTS + 1 and len(S.records(got)) == 2 and got["n_events"] == 3
    if name == "last_record":
        assert got["events"][:got["n_events"]].tolist() == [11]
    if name == "many_records":
        assert len(S.records(got)) > 4
    if name in ("n65", "n70"):
        N = got["n_corr"]
        assert not (got["bits"][:, N >> 5] >> np.uint32(N & 31)).any()       # tail bits are 0


def _bad_match(s, kp_rank, value):
    b = dict(s, f_match=s["f_match"].copy())
    b["f_match"][s["kp"][kp_rank]] = value
    return b


@pytest.mark.gpu
def test_gpu_batch_with_bad_records_equals_each_candidate_alone(gpu):
    """Five launches for any number of candidates; a record the device refuses (n > max_kf_n), a match index out of range or an octave
    outside the context's levels reports ORBFE_ERR_INVALID in its own row and changes no other row."""
    api, ctx, st = gpu
    a, b, c3 = S.batch_scenes()
    high, low = _bad_match(a, 5, len(a["valid"])), _bad_match(b, 7, -2)
    scenes = [a, high, b, c3, low, a]
    _set_frame(ctx, a["keys"])
    batch = _Batch(api, ctx, scenes, rec_n={5: 97})
    batch.enqueue(ctx, st)
    st.synchronize()
    got = [_crop(g, a["capacity"]) for g in batch.fetch()]
    refs = [M.run(s) for s in scenes[:5]] + [M.run(dict(a, refused=True))]
    for c, (g, r) in enumerate(zip(got, refs)):
        _assert_same(g, r, "candidate %d" % c)
    assert [g["status"] for g in got] == [0, M.ERR_INVALID, 0, 0, M.ERR_INVALID, M.ERR_INVALID]
    assert got[1]["n_corr"] == got[0]["n_corr"] - 1 and got[4]["n_corr"] == got[2]["n_corr"] - 1 and got[5]["n_corr"] == 0 and got[5]["n_its"] == 0
    for c in (0, 2, 3):
        one = _Batch(api, ctx, [scenes[c]])
        one.enqueue(ctx, st)
        st.synchronize()
        _assert_same(_crop(one.fetch()[0], a["capacity"]), got[c], "candidate %d alone" % c)
    again = _Batch(api, ctx, scenes, rec_n={5: 97})                     # and run to run
    again.enqueue(ctx, st)
    st.synchronize()
    for g, h in zip(got, again.fetch()):
        _assert_same(_crop(h, a["capacity"]), g, "second run")
    keys = a["keys"].copy()                                             # an octave outside the levels: that keypoint is dropped
    keys["octave"][a["kp"][3]] = S.NLEVELS
    _set_frame(ctx, keys)
    odd = _Batch(api, ctx, [a, b])
    odd.enqueue(ctx, st)
    st.synchronize()
    g = [_crop(x, a["capacity"]) for x in odd.fetch()]
    _assert_same(g[0], M.run(dict(a, keys=keys)), "octave")
    assert g[0]["status"] == M.ERR_INVALID and g[0]["n_corr"] == got[0]["n_corr"] - 1
    _assert_same(g[1], got[2], "the other candidate")


@pytest.mark.gpu
def test_gpu_sets_are_optional_and_calls_queued_on_one_stream_equal_each_alone(gpu):
    api, ctx, st = gpu
    a, b, c3 = S.batch_scenes()
    _set_frame(ctx, a["keys"])
    calls = [_Batch(api, ctx, [s], with_sets=(i != 1)) for i, s in enumerate((a, b, c3, a))]   # the scratch is reused between calls without a host wait
    for c in calls:
        c.enqueue(ctx, st)
    st.synchronize()
    for s, c in zip((a, b, c3, a), calls):
        _assert_same(_crop(c.fetch()[0], s["capacity"]), M.run(s), "queued")


@pytest.mark.gpu
def test_gpu_synchronous_form_equals_the_enqueue_form(gpu):
    api, ctx, st = gpu
    for name in ("n65", "invalid_points", "below_min", "degenerate", "many_records"):
        s = S.scene(name)
        got = ctx.pnp_ransac(s["keys"], s["f_match"], s["pos"], s["valid"], s["draws"], s["min_inliers"], s["max_its"], s["n_iterations"], s["epsilon"], s["th2"],
                             s["its_for_n"])
        _assert_same(got, _crop(_alone(gpu, s), s["capacity"]), name)
        _assert_same(got, S.model(name), name)
    s = S.scene("below_min")                                           # a frame without a keypoint, a keyframe without a slot: every padded array of the call is empty
    s = dict(s, **{k: s[k][:0] for k in ("keys", "f_match", "pos", "valid")}, capacity=1)
    got = ctx.pnp_ransac(s["keys"], s["f_match"], s["pos"], s["valid"], s["draws"], s["min_inliers"], s["max_its"], s["n_iterations"], s["epsilon"], s["th2"], s["its_for_n"])
    _assert_same(got, M.run(s), "empty")
    assert got["n_corr"] == 0 and got["n_its"] == 0 and got["n_events"] == 0 and got["exhausted"] == -1 and (got["corr"] == -1).all()
    s = _bad_match(S.scene("n65"), 5, 4000)                            # what only the device sees comes back as the call's error
    with pytest.raises(api.OrbfeError) as e:
        ctx.pnp_ransac(s["keys"], s["f_match"], s["pos"], s["valid"], s["draws"], s["min_inliers"], s["max_its"], s["n_iterations"], s["epsilon"], s["th2"], s["its_for_n"])
    assert e.value.code == api.ERR_INVALID
    with pytest.raises(api.OrbfeError):
        ctx.pnp_ransac(s["keys"], s["f_match"], s["pos"], s["valid"], s["draws"], 10, 12, 5, 0.5, 5.991, s["its_for_n"], min_set=5)


@pytest.mark.gpu
def test_gpu_bad_arguments_are_refused_and_queue_nothing(gpu):
    api, ctx, st = gpu
    s = S.batch_scenes()[0]
    _set_frame(ctx, s["keys"])
    b = _Batch(api, ctx, [s])
    for kw in (dict(slot=-1), dict(slot=64), dict(cands=0), dict(table=0), dict(n_cands=-1), dict(n_cands=65536), dict(max_kf_n=-1), dict(max_kf_n=65536),
               dict(min_set=3), dict(min_set=5), dict(min_inliers=0), dict(max_its=0), dict(max_its=-1), dict(n_iterations=-1), dict(epsilon=-0.5),
               dict(epsilon=float("nan")), dict(th2=float("inf")), dict(n_corr=0), dict(n_its=0), dict(corr=0), dict(hyp=0), dict(bits=0), dict(refined=0),
               dict(refined_bits=0), dict(events=0), dict(n_events=0), dict(exhausted=0), dict(status=0)):
        with pytest.raises(api.OrbfeError) as e:
            b.enqueue(ctx, st, **kw)
        assert e.value.code == api.ERR_INVALID, kw
    b.enqueue(ctx, st, n_cands=0)                                       # ORBFE_OK, nothing queued
    st.synchronize()
    assert b.untouched()


class _Select:
    def __init__(self, cap):
        self.T, self.cur, self.has, self.status = Guarded(np.full(16, -7.0, np.float32)), Guarded.cells(cap), Guarded(np.full(cap, HAS_UNTOUCHED, np.uint8)), Guarded.cells(1)

    def enqueue(self, ctx, st, b, c, which, k, **kw):
        o = b.out
        a = dict(slot=0, n_cands=b.n, c=c, which=which, k=k, max_its=b.max_its, n_corr=o["n_corr"].ptr, n_its=o["n_its"].ptr, corr=o["corr"].ptr, hyp=o["hyp"].ptr,
                 bits=o["bits"].ptr, refined=o["refined"].ptr, refined_bits=o["refined_bits"].ptr, exhausted=o["exhausted"].ptr, T=self.T.ptr, cur=self.cur.ptr,
                 has=self.has.ptr, status=self.status.ptr)
        a.update(kw)
        ctx.enqueue_pnp_ransac_select(a["slot"], a["n_cands"], a["c"], a["which"], a["k"], a["max_its"], a["n_corr"], a["n_its"], a["corr"], a["hyp"], a["bits"],
                                      a["refined"], a["refined_bits"], a["exhausted"], a["T"], a["cur"], a["has"], a["status"], stream=st.cuda_stream)

    def fetch(self):
        return self.T.fetch(), self.cur.fetch(), self.has.fetch(), int(self.status.fetch()[0])

    def untouched(self):
        return all(g.untouched() for g in (self.T, self.cur, self.has, self.status))


@pytest.mark.gpu
def test_gpu_select_rows_equal_the_model(gpu):
    api, ctx, st = gpu
    scenes = S.batch_scenes()
    n_keys, cap = len(scenes[0]["keys"]), ctx.capacity
    _set_frame(ctx, scenes[0]["keys"])
    batch = _Batch(api, ctx, scenes)
    batch.enqueue(ctx, st)                                              # no host wait between the calls
    refs = [M.run(s) for s in scenes]
    assert all(r["n_events"] > 0 for r in refs)
    picks = [(c, M.EVENT, int(r["events"][0])) for c, r in enumerate(refs)] + [(0, M.EVENT, int(refs[0]["events"][refs[0]["n_events"] - 1])), (1, M.EXHAUSTED, 0),
                                                                              (2, M.EXHAUSTED, 7), (0, M.EVENT, 0 if refs[0]["events"][0] > 0 else 11)]
    sels = [_Select(cap) for _ in picks]
    for sel, (c, which, k) in zip(sels, picks):
        sel.enqueue(ctx, st, batch, c, which, k)
    st.synchronize()
    for sel, (c, which, k) in zip(sels, picks):
        want = M.select_rows(refs[c], which, k, n_keys, cap, UNTOUCHED, HAS_UNTOUCHED)
        got = sel.fetch()
        assert got[3] == want[3] and got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (c, which, k)
        if want[3] == 0:
            assert got[2][:n_keys].sum() > 10 and (got[1][n_keys:] == UNTOUCHED).all()
    small = S.scene("below_min")                                        # nothing to select: the status, the identity, no point held
    _set_frame(ctx, small["keys"])
    b2 = _Batch(api, ctx, [small])
    b2.enqueue(ctx, st)
    none = [_Select(cap), _Select(cap)]
    none[0].enqueue(ctx, st, b2, 0, M.EXHAUSTED, 0)
    none[1].enqueue(ctx, st, b2, 0, M.EVENT, 5)
    st.synchronize()
    for sel in none:
        T, cur, has, status = sel.fetch()
        assert status == M.ERR_INVALID and np.array_equal(T.reshape(4, 4), np.eye(4, dtype=np.float32)) and (cur[:96] == -1).all() and not has[:96].any()
    fresh = _Select(cap)
    for kw in (dict(c=-1), dict(c=1), dict(k=-1), dict(k=12), dict(which=2), dict(slot=-1), dict(max_its=0), dict(n_corr=0), dict(hyp=0), dict(refined=0), dict(T=0),
               dict(cur=0), dict(has=0), dict(status=0)):
        with pytest.raises(api.OrbfeError) as e:
            fresh.enqueue(ctx, st, b2, kw.pop("c", 0), kw.pop("which", M.EVENT), kw.pop("k", 0), **kw)
        assert e.value.code == api.ERR_INVALID, kw
    st.synchronize()
    assert fresh.untouched()


@pytest.mark.gpu
def test_gpu_select_then_pose_optimization_without_uploads_equals_the_upload_path(gpu):
    """batch -> (one download of the events) -> select -> orbfe_enqueue_pose_optimization on one stream against the existing path: the
    same pose call fed by host uploads of the 4 x 4 pose and the masked has_point row that the model forms from the fetched rows.  The
    pose, the outlier flags and the inlier count are bit-equal."""
    import torch
    api, ctx, st = gpu
    s = S.scene("clean")
    n_keys, cap = len(s["keys"]), ctx.capacity
    _set_frame(ctx, s["keys"])
    bufs = device_buffers(ctx)
    Xw = np.zeros((cap, 3), np.float32)                                 # the BoW batch's d_Xw row: the matched point of every matched keypoint
    held = s["f_match"] >= 0
    Xw[:n_keys][held] = s["pos"][s["f_match"][held]]
    own = []
    d_Xw = _up(own, Xw)
    d_off = upload(np.array([0, n_keys], np.int32))[0]
    d_keys = ctx.device_keys_un(0, st.cuda_stream)

    def pose(d_T, d_has):
        outl, n_in = Guarded(np.zeros(cap, np.uint8)), Guarded.cells(1)
        ctx._check(ctx.L.orbfe_enqueue_pose_optimization(ctx.h, 1, d_off.data_ptr(), d_keys, bufs["u_right"], d_has, d_Xw, d_T, outl.ptr, n_in.ptr, cap,
                                                         st.cuda_stream))
        return outl, n_in

    batch = _Batch(api, ctx, [s])
    batch.enqueue(ctx, st)
    st.synchronize()                                                    # the one download: the events
    rows = batch.fetch()[0]
    assert rows["n_events"] > 0
    k = int(rows["events"][0])
    sel = _Select(cap)
    sel.enqueue(ctx, st, batch, 0, M.EVENT, k)
    dev = pose(sel.T.ptr, sel.has.ptr)
    st.synchronize()
    ref = S.model("clean")                                              # the upload path is fed the MODEL's rows, not the device's
    assert ref["n_events"] > 0 and int(ref["events"][0]) == k
    T0, cur, has, status = M.select_rows(ref, M.EVENT, k, n_keys, cap, UNTOUCHED, 0)
    assert status == 0
    up_T = Guarded(T0)
    host = pose(up_T.ptr, _up(own, has))
    st.synchronize()
    print("event %d: %d refined inliers, PoseOptimization kept %d" % (k, has.sum(), dev[1].fetch()[0]))
    assert sel.T.fetch().tobytes() == up_T.fetch().tobytes() and not np.array_equal(up_T.fetch(), T0)   # the pose call moved it, equally
    assert dev[0].fetch().tobytes() == host[0].fetch().tobytes() and dev[1].fetch()[0] == host[1].fetch()[0] > 20
