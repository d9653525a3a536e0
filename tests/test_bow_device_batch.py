"""SearchByFboW(KeyFrame*, Frame&) against all relocalisation candidates in one call (orbfe_enqueue_search_by_bow_batch;
orbslam2_amd/csrc/orbfe_bow_device.hip): a device array of orbfe_bow_keyframe records in, one row of every output per keyframe.
Every comparison is exact: row k against the CPU oracle AND, bit for bit, against orbfe_enqueue_search_by_bow on keyframe k alone.

The frame is the 1600-descriptor frame of tests/test_bow_device.py (_scene), the vocabulary its small one (k = 10, 5 levels).  The
candidate family (_family) is chosen so that no two rows agree -- an implementation that mixes up keyframe indices or output rows
cannot pass -- and so that the order inside a node matters for two of its members.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from orbslam2_amd import bow as B
from tests import test_bow as TB
from tests import test_bow_device as TD
from tests.device_arrays import HAS_UNTOUCHED, UNTOUCHED, XW_UNTOUCHED, Guarded, context, upload, upload_records

NAMES = ["scene", "c11", "c12", "tiny", "self", "novalid"]
SETTINGS = ((0.7, True), (0.9, False))


# ------------------------------------------------------------------ the candidate family (CPU)
def _cand(f_d, f_ang, seed, n_copy, n_noise, flip, pvalid, dang):
    rng = np.random.default_rng(seed)
    perm = rng.permutation(len(f_d))[:n_copy]
    d = np.concatenate([TB._descs(seed + 100, 0, base=f_d[perm], flip=flip), TB._descs(seed + 200, n_noise)])
    valid = (rng.random(len(d)) < pvalid).astype(np.int32)
    ang = np.concatenate([(f_ang[perm] + rng.normal(0, dang, n_copy)) % 360, rng.uniform(0, 360, n_noise)]).astype(np.float32)
    ang[ang >= 360] = 0  # a double just below 360 may round up to it
    return dict(d=np.ascontiguousarray(d), valid=valid, ang=ang)


_CACHE = {}


def _frame():
    if "frame" not in _CACHE:
        sc = TD._scene()
        assert len(sc["f_d"]) == 1600
        fam = {
            "scene": dict(d=sc["kf_d"], valid=sc["kf_valid"], ang=sc["kf_ang"]),
            "c11": _cand(sc["f_d"], sc["f_ang"], 11, 900, 300, 0.02, 0.9, 5),
            "c12": _cand(sc["f_d"], sc["f_ang"], 12, 1300, 700, 0.06, 0.7, 40),
            "tiny": _cand(sc["f_d"], sc["f_ang"], 13, 40, 0, 0.03, 1.0, 3),
            "self": dict(d=sc["f_d"], valid=np.ones(1600, np.int32), ang=sc["f_ang"]),
            "novalid": dict(d=sc["kf_d"], valid=np.zeros_like(sc["kf_valid"]), ang=sc["kf_ang"]),
        }
        _CACHE["frame"] = (sc, fam)
    return _CACHE["frame"]


def _search(L, kf, f_fv, f_d, f_ang, ratio, ori):
    return TD._oracle_search(L, kf["fv"], kf["valid"], kf["d"], kf["ang"], f_fv, f_d, f_ang, ratio, ori)


def _family(level):
    """The family at `level`, computed once: per member its feature vector and the oracle's (matches, count) per setting."""
    if level not in _CACHE:
        sc, fam = _frame()
        L, v = TB._oracle_voc(sc["vocab"])
        per, fbow, f_fv = TB._oracle_transform(L, v, sc["f_d"], level)
        kfs = []
        for name in NAMES:
            kf = dict(fam[name], name=name)
            kf["fv"] = TB._oracle_transform(L, v, kf["d"], level)[2]
            kf["ref"] = {s: _search(L, kf, f_fv, sc["f_d"], sc["f_ang"], *s) for s in SETTINGS}
            kfs.append(kf)
        L.orc_vocab_destroy(v)
        _CACHE[level] = dict(sc=sc, per=per, fbow=fbow, f_fv=f_fv, kfs=kfs)
    return _CACHE[level]


# ------------------------------------------------------------------ CPU
def test_the_library_exports_the_batch_call_and_the_keyframe_record():
    from orbslam2_amd import api
    L = api.load()
    name = "orbfe_enqueue_search_by_bow_batch"
    assert name in api.EXPORTS
    fn = getattr(L, name)  # AttributeError: the symbol is not exported
    args = [0 if t is C.c_int else 0.0 if t is C.c_float else None for t in fn.argtypes]
    assert fn(*args) == api.ERR_INVALID
    assert callable(api.Context.enqueue_search_by_bow_batch)
    assert C.sizeof(api.BowKeyframe) == 64


def test_the_candidate_family_tells_rows_and_in_node_order_apart():
    """Oracle only: every member finds what its construction promises, any two rows differ at both levels and settings, and the
    `no blocking` variant (tests/test_bow_device.py) differs from the oracle for `scene` and `c11`."""
    floors = dict(scene=lambda n: n > 300, c11=lambda n: n > 300, c12=lambda n: n > 150, tiny=lambda n: n >= 15, self=lambda n: n == 1600,
                  novalid=lambda n: n == 0)
    for level in (4, 2):
        fam = _family(level)
        sc = fam["sc"]
        for s in SETTINGS:
            rows = [kf["ref"][s][0] for kf in fam["kfs"]]
            counts = [kf["ref"][s][1] for kf in fam["kfs"]]
            print("level %d %s: nref %s, nodes %s" % (level, s, counts, [len(kf["fv"][0]) for kf in fam["kfs"]]))
            for kf, n in zip(fam["kfs"], counts):
                assert floors[kf["name"]](n), (level, s, kf["name"], n)
            for i in range(len(rows)):
                for j in range(i):
                    assert (rows[i] != rows[j]).any(), (level, s, NAMES[i], NAMES[j])
            print("    any two rows differ in at least %d entries" % min(int((rows[i] != rows[j]).sum()) for i in range(len(rows)) for j in range(i)))
        for kf in fam["kfs"][:2]:
            for ratio, _ in SETTINGS:
                plain, _ = _search(O.lib(), kf, fam["f_fv"], sc["f_d"], sc["f_ang"], ratio, False)
                var = TD._no_blocking_variant(kf["fv"], kf["valid"], kf["d"], fam["f_fv"], sc["f_d"], ratio)
                assert (var != plain).any(), (level, kf["name"], ratio)
    # what the edge cases of the GPU tests rely on at level 4
    nn = {kf["name"]: len(kf["fv"][0]) for kf in _family(4)["kfs"]}
    assert sorted(k for k, n in nn.items() if n > 300) == ["c11", "c12", "self"], nn


# ------------------------------------------------------------------ helpers (GPU)
def _kf_dev(kf, pos=None):
    return TD._Kf(kf["fv"], kf["valid"], kf["d"], kf["ang"], pos)


def _pos(kf, seed):
    return np.random.default_rng(seed).uniform(-5, 5, (len(kf["d"]), 3)).astype(np.float32)


def _record(api, kf, nnodes=None):
    p = [t.data_ptr() if t.numel() else None for t in kf.keep]
    return api.BowKeyframe(p[0], p[1], p[2], p[3], p[4], p[5], None if kf.pos is None else kf.pos.data_ptr(), kf.nnodes if nnodes is None else nnodes, kf.n)


class _Rows:
    """K rows of outputs between guards, every cell holding a sentinel; filled by one batch call or row by row by the single call."""

    def __init__(self, cap, K, pose=False):
        self.cap, self.K = cap, K
        self.match, self.nm, self.status = Guarded.cells(max(K, 1) * cap), Guarded.cells(max(K, 1)), Guarded.cells(max(K, 1))
        self.has = Guarded(np.full(max(K, 1) * cap, HAS_UNTOUCHED, np.uint8)) if pose else None
        self.Xw = Guarded(np.full(max(K, 1) * cap * 3, XW_UNTOUCHED, np.float32)) if pose else None

    def batch(self, ctx, d_recs, max_nn, fv, ratio, ori, st, n_kfs=None, slot=0):
        ctx.enqueue_search_by_bow_batch(slot, d_recs.data_ptr() if d_recs is not None and d_recs.numel() else 0, self.K if n_kfs is None else n_kfs, max_nn,
                                        fv.nodes.ptr, fv.node_off.ptr, fv.node_feat.ptr, fv.n_nodes.ptr, ratio, ori,
                                        self.match.ptr, self.nm.ptr, self.status.ptr,
                                        d_has_point=0 if self.has is None else self.has.ptr, d_Xw=0 if self.Xw is None else self.Xw.ptr,
                                        stream=st.cuda_stream)

    def single(self, ctx, k, kf, fv, ratio, ori, st):
        p = [t.data_ptr() if t.numel() else 0 for t in kf.keep]
        cap = self.cap
        ctx.enqueue_search_by_bow(0, p[0], p[1], p[2], kf.nnodes, p[3], p[4], p[5], kf.n,
                                  fv.nodes.ptr, fv.node_off.ptr, fv.node_feat.ptr, fv.n_nodes.ptr, ratio, ori,
                                  self.match.ptr + 4 * k * cap, self.nm.ptr + 4 * k, self.status.ptr + 4 * k,
                                  d_kf_pos=0 if kf.pos is None else kf.pos.data_ptr(), d_has_point=0 if self.has is None else self.has.ptr + k * cap,
                                  d_Xw=0 if self.Xw is None else self.Xw.ptr + 12 * k * cap, stream=st.cuda_stream)

    def fetch(self):
        out = dict(match=TD._np(self.match).reshape(-1, self.cap), nm=TD._np(self.nm), status=TD._np(self.status))
        if self.has is not None:
            out["has"] = self.has.fetch().reshape(-1, self.cap)
            out["Xw"] = self.Xw.fetch().reshape(-1, self.cap, 3)
        return out

    def check_row(self, got, k, ref, nref, what=""):
        n = len(ref)
        assert got["status"][k] == 0, (what, k)
        assert got["nm"][k] == nref, (what, k, int(got["nm"][k]), nref)
        assert np.array_equal(got["match"][k, :n], ref), (what, k, int((got["match"][k, :n] != ref).sum()))
        assert (got["match"][k, n:] == UNTOUCHED).all(), (what, k)

    def untouched(self):
        got = self.fetch()
        ok = (got["match"] == UNTOUCHED).all() and (got["nm"] == UNTOUCHED).all() and (got["status"] == UNTOUCHED).all()
        if self.has is not None:
            ok = ok and (got["has"] == HAS_UNTOUCHED).all() and (got["Xw"] == XW_UNTOUCHED).all()
        return bool(ok)


def _same(a, b):
    """Two fetched output sets are the same bit for bit (floats by their bits)."""
    return a.keys() == b.keys() and all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)) for k in a)


def _setup(api, level):
    """Context with the vocabulary, the frame injected into slot 0, its feature vector queued on a fresh stream."""
    import torch
    fam = _family(level)
    sc = fam["sc"]
    ctx = context(api)
    B.vocab_load(ctx, sc["vocab"])
    TD._inject_desc(ctx, sc["f_d"], sc["f_ang"])
    st = torch.cuda.Stream()
    fv = TD._Fv(ctx.capacity)
    torch.cuda.synchronize()
    fv.enqueue(ctx, 0, level, st)
    return fam, ctx, st, fv


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("level", [4, 2])
def test_gpu_the_family_in_one_call(level):
    """3. Per setting one batch call with the pose outputs and the six single calls on the same stream, one synchronise: row k ==
    oracle, == the single call on keyframe k bit for bit (has_point and Xw included), untouched beyond the slot's count, status 0.
    `scene` has no pos array: its Xw row stays untouched; `c11` has one."""
    import torch
    from orbslam2_amd import api
    fam, ctx, st, fv = _setup(api, level)
    n = len(fam["sc"]["f_d"])
    kfs = [_kf_dev(kf, None if kf["name"] == "scene" else _pos(kf, 40 + i)) for i, kf in enumerate(fam["kfs"])]
    d_recs = upload_records([_record(api, kf) for kf in kfs])
    max_nn = max(kf.nnodes for kf in kfs)
    for ratio, ori in SETTINGS:
        bat, one = _Rows(ctx.capacity, len(kfs), pose=True), _Rows(ctx.capacity, len(kfs), pose=True)
        torch.cuda.synchronize()  # the sentinels are in place
        bat.batch(ctx, d_recs, max_nn, fv, ratio, ori, st)
        for k, kf in enumerate(kfs):
            one.single(ctx, k, kf, fv, ratio, ori, st)
        st.synchronize()
        got, ref = bat.fetch(), one.fetch()
        for k, kf in enumerate(fam["kfs"]):
            bat.check_row(got, k, *kf["ref"][(ratio, ori)], what=(level, ratio, kf["name"]))
            m = got["match"][k, :n]
            assert np.array_equal(got["has"][k, :n], m >= 0) and (got["has"][k, n:] == HAS_UNTOUCHED).all()
            if kfs[k].pos is None:
                assert (got["Xw"][k] == XW_UNTOUCHED).all()
            else:
                pos = kfs[k].pos.cpu().numpy().reshape(-1, 3)
                assert np.array_equal(got["Xw"][k, :n][m >= 0], pos[m[m >= 0]]) and (got["Xw"][k, :n][m < 0] == XW_UNTOUCHED).all()
                assert (got["Xw"][k, n:] == XW_UNTOUCHED).all()
        assert _same(got, ref), (level, ratio)
    fv.check(fam["per"], fam["fbow"], fam["f_fv"], level)
    ctx.close()


@pytest.mark.gpu
def test_gpu_batch_calls_queue_back_to_back_and_rows_follow_the_records():
    """4. Two batch calls with different settings, the second over the reversed family, then a single call and a one-keyframe
    batch, all on one stream with one synchronise: every row exact, the reversed batch gives the reversed rows, n_kfs == 1 equals
    the single call."""
    import torch
    from orbslam2_amd import api
    fam, ctx, st, fv = _setup(api, 4)
    kfs = [_kf_dev(kf) for kf in fam["kfs"]]
    K = len(kfs)
    fwd = upload_records([_record(api, kf) for kf in kfs])
    rev = upload_records([_record(api, kf) for kf in kfs[::-1]])
    max_nn = max(kf.nnodes for kf in kfs)
    a, b, c = _Rows(ctx.capacity, K), _Rows(ctx.capacity, K), _Rows(ctx.capacity, K)
    one, one_b = _Rows(ctx.capacity, 1), _Rows(ctx.capacity, 1)
    just_one = upload_records([_record(api, kfs[1])])
    torch.cuda.synchronize()  # the sentinels and records are in place; from here on nothing waits until the one synchronise
    a.batch(ctx, fwd, max_nn, fv, *SETTINGS[0], st)
    b.batch(ctx, rev, max_nn, fv, *SETTINGS[1], st)
    c.batch(ctx, rev, max_nn, fv, *SETTINGS[0], st)
    one.single(ctx, 0, kfs[1], fv, *SETTINGS[1], st)
    one_b.batch(ctx, just_one, kfs[1].nnodes, fv, *SETTINGS[1], st)
    st.synchronize()
    ga, gb, gc = a.fetch(), b.fetch(), c.fetch()
    for k, kf in enumerate(fam["kfs"]):
        a.check_row(ga, k, *kf["ref"][SETTINGS[0]], what=("a", kf["name"]))
        b.check_row(gb, K - 1 - k, *kf["ref"][SETTINGS[1]], what=("b", kf["name"]))
    assert _same({k: v[::-1] for k, v in gc.items()}, ga)
    g1 = one.fetch()
    one.check_row(g1, 0, *fam["kfs"][1]["ref"][SETTINGS[1]], what="single")
    assert _same(one_b.fetch(), g1)
    ctx.close()


@pytest.mark.gpu
def test_gpu_more_keyframes_than_a_wave_has_lanes():
    """5. 70 small keyframes (n_kfs > 64), max_kf_nnodes from the data: every row == oracle."""
    import torch
    from orbslam2_amd import api
    fam, ctx, st, fv = _setup(api, 4)
    sc = fam["sc"]
    L, v = TB._oracle_voc(sc["vocab"])
    cands, kfs = [], []
    for k in range(70):
        kf = _cand(sc["f_d"], sc["f_ang"], 300 + k, 150, 50, 0.03, 0.85, 5)
        kf["fv"] = TB._oracle_transform(L, v, kf["d"], 4)[2]
        cands.append(kf)
        kfs.append(_kf_dev(kf))
    out, d_recs = _Rows(ctx.capacity, 70), upload_records([_record(api, kf) for kf in kfs])
    torch.cuda.synchronize()
    out.batch(ctx, d_recs, max(kf.nnodes for kf in kfs), fv, 0.7, True, st)
    st.synchronize()
    got = out.fetch()
    counts = []
    for k, kf in enumerate(cands):
        ref, nref = _search(L, kf, fam["f_fv"], sc["f_d"], sc["f_ang"], 0.7, True)
        assert nref > 30, (k, nref)
        counts.append(nref)
        out.check_row(got, k, ref, nref, what=k)
    print("70 keyframes: nref %d .. %d" % (min(counts), max(counts)))
    L.orc_vocab_destroy(v)
    ctx.close()


@pytest.mark.gpu
def test_gpu_batch_edge_cases():
    """6. What the host refuses, what only the device can see (reported per keyframe, the other rows still exact), and the empty
    cases."""
    import torch
    from orbslam2_amd import api
    from tests import test_matchers as TM
    fam = _family(4)
    sc = fam["sc"]
    s0 = SETTINGS[0]
    ctx = context(api)
    B.vocab_load(ctx, sc["vocab"])
    st = torch.cuda.Stream()
    kfs = [_kf_dev(kf) for kf in fam["kfs"]]
    K = len(kfs)
    recs = [_record(api, kf) for kf in kfs]
    max_nn = max(kf.nnodes for kf in kfs)
    # a frame without keypoints
    flat = np.full((TM.H, TM.W), 128, np.uint8)
    assert len(ctx.stereo_frame(flat, flat)["kps_left"]) == 0
    fv, out, d_recs = TD._Fv(ctx.capacity), _Rows(ctx.capacity, K, pose=True), upload_records(recs)
    torch.cuda.synchronize()
    fv.enqueue(ctx, 0, 4, st)
    out.batch(ctx, d_recs, max_nn, fv, *s0, st)
    st.synchronize()
    got = out.fetch()
    assert (got["status"] == api.ERR_INVALID).all() and (got["nm"] == 0).all() and (got["match"] == UNTOUCHED).all()
    assert (got["has"] == HAS_UNTOUCHED).all() and (got["Xw"] == XW_UNTOUCHED).all()
    # the scene
    TD._inject_desc(ctx, sc["f_d"], sc["f_ang"])
    n = len(sc["f_d"])
    fv = TD._Fv(ctx.capacity)
    torch.cuda.synchronize()
    fv.enqueue(ctx, 0, 4, st)

    def run(rs, bound, refused=(), other=(), what=""):
        out, d_rs = _Rows(ctx.capacity, len(rs)), upload_records(rs)
        torch.cuda.synchronize()
        out.batch(ctx, d_rs, bound, fv, *s0, st)
        st.synchronize()
        got = out.fetch()
        for k, kf in enumerate(fam["kfs"][: len(rs)]):
            if kf["name"] in refused:
                assert got["status"][k] == api.ERR_INVALID, (what, kf["name"])
            elif kf["name"] not in other:
                out.check_row(got, k, *kf["ref"][s0], what=(what, kf["name"]))
        return got

    # n_kfs == 0: OK, nothing queued (with and without a record array)
    out = _Rows(ctx.capacity, 2, pose=True)
    torch.cuda.synchronize()
    out.batch(ctx, None, max_nn, fv, *s0, st, n_kfs=0)
    out.batch(ctx, d_recs, max_nn, fv, *s0, st, n_kfs=0)
    st.synchronize()
    assert out.untouched()
    # a bound below some node counts: those keyframes are refused, none is searched in part
    run(recs, 300, refused=("c11", "c12", "self"), what="max_kf_nnodes = 300")
    run(recs, 0, refused=NAMES, what="max_kf_nnodes = 0")
    # nnodes = -1 in one record
    bad = list(recs); bad[1] = _record(api, kfs[1], nnodes=-1)
    run(bad, max_nn, refused=("c11",), what="nnodes = -1")
    # two nodes swapped
    kf2 = fam["kfs"][2]
    j = 5
    nodes = kf2["fv"][0].copy(); nodes[[j, j + 1]] = nodes[[j + 1, j]]
    swapped = TD._Kf((nodes, kf2["fv"][1], kf2["fv"][2]), kf2["valid"], kf2["d"], kf2["ang"])
    bad = list(recs); bad[2] = _record(api, swapped)
    run(bad, max_nn, refused=("c12",), what="nodes swapped")
    # a KF feature index out of range, in a node the frame shares
    kf0 = fam["kfs"][0]
    shared = np.nonzero(np.isin(kf0["fv"][0], fam["f_fv"][0]))[0]
    feat = kf0["fv"][2].copy(); feat[kf0["fv"][1][shared[3]]] = len(kf0["d"]) + 5
    broken = TD._Kf((kf0["fv"][0], kf0["fv"][1], feat), kf0["valid"], kf0["d"], kf0["ang"])
    bad = list(recs); bad[0] = _record(api, broken)
    run(bad, max_nn, refused=("scene",), what="feature index")
    # a record without nodes and without arrays: no match, no complaint
    bad = list(recs); bad[4] = api.BowKeyframe(None, None, None, None, None, None, None, 0, 0)
    got = run(bad, max_nn, other=("self",), what="empty record")
    assert got["status"][4] == 0 and got["nm"][4] == 0 and (got["match"][4, :n] == -1).all() and (got["match"][4, n:] == UNTOUCHED).all()
    # what the host sees: refused, nothing queued
    out = _Rows(ctx.capacity, K, pose=True)
    torch.cuda.synchronize()
    for kw in (dict(d_recs=None), dict(d_recs=d_recs, slot=7), dict(d_recs=d_recs, slot=-1), dict(d_recs=d_recs, n_kfs=-1), dict(d_recs=d_recs, n_kfs=65536)):
        with pytest.raises(api.OrbfeError):
            out.batch(ctx, kw.pop("d_recs"), max_nn, fv, *s0, st, **kw)
    with pytest.raises(api.OrbfeError):
        out.batch(ctx, d_recs, -1, fv, *s0, st)
    st.synchronize()
    assert out.untouched()
    run(recs, max_nn, what="after the refusals")  # the context still works
    ctx.close()


@pytest.mark.gpu
def test_gpu_extraction_bow_and_batch_on_one_stream():
    """7. enqueue_stereo -> enqueue_compute_bow -> the batch over four perturbed copies of the frame's own descriptors, one
    synchronise, then fetch: == oracle."""
    import torch
    from orbslam2_amd import api, synth
    from tests import test_matchers as TM
    ctx = context(api, nfeatures=1500)
    blob = TD._vocab()
    B.vocab_load(ctx, blob)
    L, v = TB._oracle_voc(blob)
    left, right = synth.stereo_pair(TM.W, TM.H, seed=702)
    d_img = upload(np.stack([left, right]).astype(np.uint8))[0]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    ctx.enqueue_stereo(d_img.data_ptr(), 1, st.cuda_stream)
    ctx.synchronize(st.cuda_stream)
    fr = ctx.fetch_image(0, stereo=True)
    d, ang = np.ascontiguousarray(fr["desc"]), np.ascontiguousarray(fr["kps"]["angle"])
    assert len(d) > 300
    per, fbow, f_fv = TB._oracle_transform(L, v, d, 4)
    cands = []
    for i, flip in enumerate((0.02, 0.04, 0.06, 0.08)):
        rng = np.random.default_rng(800 + i)
        perm = rng.permutation(len(d))[: len(d) - 50 * i]
        kf = dict(d=TB._descs(810 + i, 0, base=d[perm], flip=flip), valid=(rng.random(len(perm)) < 0.9).astype(np.int32))
        kf["ang"] = ((ang[perm] + rng.normal(0, 4, len(perm))) % 360).astype(np.float32)
        kf["ang"][kf["ang"] >= 360] = 0
        kf["fv"] = TB._oracle_transform(L, v, kf["d"], 4)[2]
        cands.append(kf)
    kfs = [_kf_dev(kf) for kf in cands]
    d_recs = upload_records([_record(api, kf) for kf in kfs])
    fv, out = TD._Fv(ctx.capacity), _Rows(ctx.capacity, 4)
    torch.cuda.synchronize()
    ctx.enqueue_stereo(d_img.data_ptr(), 1, st.cuda_stream)  # nothing is fetched and nothing waits until the end
    fv.enqueue(ctx, 0, 4, st)
    out.batch(ctx, d_recs, max(kf.nnodes for kf in kfs), fv, 0.7, True, st)
    st.synchronize()
    fv.check(per, fbow, f_fv)
    got = out.fetch()
    seen = []
    for k, kf in enumerate(cands):
        ref, nref = _search(L, kf, f_fv, d, ang, 0.7, True)
        assert nref > 40, (k, nref)
        out.check_row(got, k, ref, nref, what=k)
        seen.append(nref)
    print("real frame, %d keypoints: nref %s" % (len(d), seen))
    L.orc_vocab_destroy(v)
    ctx.close()
