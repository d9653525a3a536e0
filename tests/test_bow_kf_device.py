"""ORBmatcher::SearchByFboW(KeyFrame*, KeyFrame*) (src/ORBmatcher.cc:517-650) on device-resident keyframes, one candidate or all
candidates of LoopClosing::ComputeSim3 in one call: orbfe_enqueue_search_by_bow_kf / _batch (orbslam2_amd/csrc/orbfe_bow_device.hip).
Every comparison is exact: against the CPU oracle (orc_search_by_bow_kf), on the GPU against the synchronous orbfe_search_by_bow_kf as
well, and a batch row against the single call bit for bit.  Scenes, oracle binding, variants and census are in tests/bow_kf_scenes.py.

Device arrays are torch tensors, every input over-allocated by PAD zero entries (a check the kernel misses then reads inside the
test's own allocation and shows as a wrong status or result), every output surrounded by GUARD sentinel cells; the stream is never
the default one.
"""
import ctypes as C

import numpy as np
import pytest

from orbslam2_amd import bow as B
from tests import bow_kf_scenes as S
from tests.device_arrays import UNTOUCHED, Guarded, context, upload, upload_records

NAMES = ["orbfe_enqueue_search_by_bow_kf", "orbfe_enqueue_search_by_bow_kf_batch"]
PAD = 64
FLOORS = dict(pos64=20, pos128=20, pos4096=8, second_round=1, flag_changed=10, valid2_changed=10, at_th_low=10, tie_rejected=10, pruned=5,
              only_kf1=1, only_kf2=1)


# ------------------------------------------------------------------ CPU
def test_the_library_exports_both_calls_and_they_refuse_a_null_context():
    """a. Fails on a library without the calls."""
    from orbslam2_amd import api
    L = api.load()
    for name in NAMES:
        assert name in api.EXPORTS
        fn = getattr(L, name)  # AttributeError: the symbol is not exported
        args = [0 if t is C.c_int else 0.0 if t is C.c_float else None for t in fn.argtypes]
        assert fn(*args) == api.ERR_INVALID
    assert callable(api.Context.enqueue_search_by_bow_kf) and callable(api.Context.enqueue_search_by_bow_kf_batch)
    assert C.sizeof(api.BowKeyframe) == 64


def test_the_scenes_reach_every_class_and_every_broken_rule_shows():
    """b. Oracle only.  What keeps the GPU tests from passing on inputs that exercise nothing: over the big-node scene at (0.75, true)
    the oracle's run has winners beyond the register chunks (64, 128) and beyond the 64 flag bits (4096), a KF1 node of more than 64
    valid features, winners changed by vbMatched2 and by valid2, best distances of exactly TH_LOW that pass the ratio test, rejections
    by a tie alone, histogram losers, and nodes on one side only in both directions; and each variant that breaks one rule computes
    something else.  The census itself equals the oracle on every scene and setting."""
    for name, (kf1, kf2) in S.scenes().items():
        for s in S.SETTINGS:
            ref, nref = S.oracle(kf1, kf2, *s)
            got, ngot, cls = S.census(kf1, kf2, *s)
            print(name, s, nref, cls)
            assert ngot == nref and np.array_equal(got, ref), (name, s)
    kf1, kf2 = S.big_node()
    assert len(kf1["d"]) != len(kf2["d"]) and len(kf1["d"]) % 64 and len(kf2["d"]) % 64
    assert max(np.diff(kf2["fv"][1])) == 4200
    ref, nref = S.oracle(kf1, kf2, 0.75, True)
    _, _, cls = S.census(kf1, kf2, 0.75, True)
    for k, floor in FLOORS.items():
        assert cls[k] >= floor, (k, cls[k], floor)
    for variant in S.VARIANTS:
        got, _, _ = S.census(kf1, kf2, 0.75, True, variant=variant)
        print(variant, "differs from the oracle in", int((got != ref).sum()), "entries")
        assert (got != ref).sum() >= 10, variant
    # identical descriptors: with nnratio <= 1 only a node of one KF2 keypoint accepts; above 1 the flags carry the result
    for n2 in S.NODE_SIZES:
        kf1, kf2 = S.single_node(5, n2)
        for ratio, ori in S.SETTINGS:
            ref, nref = S.oracle(kf1, kf2, ratio, ori)
            if ratio <= 1:
                assert nref == (1 if n2 == 1 else 0) and (n2 > 1 or ref[0] == 0), (n2, ratio)
            else:
                assert nref == min(5, n2) and np.array_equal(ref[:nref], np.arange(nref)), (n2, ratio)


def test_the_oracle_equals_the_literal_transcription_on_every_scene():
    """c."""
    for name, (kf1, kf2) in S.scenes().items():
        for s in S.SETTINGS:
            ref, nref = S.oracle(kf1, kf2, *s)
            lit, nlit = S.literal(kf1, kf2, *s)
            assert nlit == nref and np.array_equal(lit, ref), (name, s)


def test_the_candidate_family_tells_rows_apart():
    """d. Oracle only: every member finds what its construction promises, any two rows differ, and the big candidate's winners lie
    beyond list position 4096."""
    kf1, fam = S.family()
    assert len(kf1["d"]) == 1500 and max(len(k["d"]) for k in fam) > 4096
    floors = dict(perturbed=lambda n: n > 300, sparse=lambda n: n > 20, tiny=lambda n: n >= 10, self=lambda n: n > 1000, novalid=lambda n: n == 0,
                  big=lambda n: n > 150)
    for s in S.SETTINGS:
        rows = [S.oracle(kf1, kf, *s) for kf in fam]
        print(s, [r[1] for r in rows])
        for name, (_, n) in zip(S.FAMILY, rows):
            assert floors[name](n), (s, name, n)
        for i in range(len(rows)):
            for j in range(i):
                assert (rows[i][0] != rows[j][0]).any(), (s, S.FAMILY[i], S.FAMILY[j])
        got, ngot, cls = S.census(kf1, fam[-1], *s)
        assert ngot == rows[-1][1] and np.array_equal(got, rows[-1][0]) and cls["pos4096"] >= 20 and cls["flag_changed"] >= 10, (s, cls)
    own = S.oracle(kf1, kf1, 0.75, True)[0]
    assert np.array_equal(own[own >= 0], np.nonzero(own >= 0)[0])  # a keyframe against itself matches keypoint i with keypoint i


# ------------------------------------------------------------------ helpers (GPU)
class _Kf:
    """A keyframe's arrays in HBM and its record.  Edits (name -> array) replace arrays before the upload."""

    ORDER = ("nodes", "off", "feat", "valid", "desc", "angle")

    def __init__(self, api, kf, nnodes=None, n=None, **edits):
        a = dict(nodes=kf["fv"][0], off=kf["fv"][1], feat=kf["fv"][2], valid=kf["valid"], desc=kf["d"].reshape(-1), angle=kf["ang"])
        a.update(edits)
        self.t = {k: upload(v, pad=PAD) for k, v in a.items()}
        self.n = len(kf["d"]) if n is None else n
        self.nnodes = len(kf["fv"][0]) if nnodes is None else nnodes
        self.rec = api.BowKeyframe(*[self.t[k][1] for k in self.ORDER], None, self.nnodes, self.n)


def _rec_array(kfs):
    return upload_records(kf.rec if isinstance(kf, _Kf) else kf for kf in kfs)


class _Out:
    """K rows of outputs between guards: match12[K][n1], pairs[K][2 * n1], count[K], status[K]."""

    def __init__(self, n1, K=1):
        self.n1, self.K = n1, K
        self.sizes = (K * n1, K * 2 * n1, K, K)
        self.g = [Guarded.cells(s) for s in self.sizes]

    def ptr(self, k, row=0):
        return self.g[k].ptr + 4 * row * (self.sizes[k] // self.K)

    def single(self, ctx, k1, k2, ratio, ori, st, pairs=True, row=0):
        ctx.enqueue_search_by_bow_kf(k1 if k1 is None or not isinstance(k1, _Kf) else k1.rec, k2 if k2 is None or not isinstance(k2, _Kf) else k2.rec,
                                     ratio, ori, self.ptr(0, row), self.ptr(2, row), self.ptr(3, row), d_pairs=self.ptr(1, row) if pairs else 0,
                                     stream=st.cuda_stream)

    def batch(self, ctx, k1, d_recs, max_kf_n, ratio, ori, st, pairs=True, n_kfs=None):
        ctx.enqueue_search_by_bow_kf_batch(k1 if k1 is None or not isinstance(k1, _Kf) else k1.rec, d_recs.data_ptr() if d_recs is not None else 0,
                                           self.K if n_kfs is None else n_kfs, max_kf_n, ratio, ori, self.ptr(0), self.ptr(2), self.ptr(3),
                                           d_pairs=self.ptr(1) if pairs else 0, stream=st.cuda_stream)

    def fetch(self):
        """(match12[K][n1], pairs[K][2 * n1], count[K], status[K]); asserts that every cell outside them still holds the sentinel."""
        return [g.fetch().reshape(self.K, s // self.K) for g, s in zip(self.g, self.sizes)]

    def untouched(self):
        return all(g.untouched() for g in self.g)


def _check_row(got, k, ref, nref, pairs=True, what=""):
    m, p, nm, status = (g[k] for g in got)
    assert status[0] == 0, (what, k, int(status[0]))
    assert nm[0] == nref, (what, k, int(nm[0]), nref)
    assert np.array_equal(m, ref), (what, k, int((m != ref).sum()))
    if pairs:
        assert np.array_equal(p[:2 * nref], S.pairs_of(ref)), (what, k)
        assert (p[2 * nref:] == UNTOUCHED).all(), (what, k)
    else:
        assert (p == UNTOUCHED).all(), (what, k)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _sync(ctx, kf1, kf2, ratio, ori):
    return B.search_by_bow_kf(ctx, kf1["fv"], kf1["valid"], kf1["d"], kf1["ang"], kf2["fv"], kf2["valid"], kf2["d"], kf2["ang"], ratio, ori)


def _edit(arr, at, value):
    out = arr.copy()
    out[at] = value
    return out


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_gpu_every_scene_through_the_single_call():
    """1. Every scene and setting: match12, count and pairs equal the oracle and the synchronous call, status 0, entries past
    2 * count and the guards untouched; without d_pairs the other outputs are the same.  The calls run back to back on one
    context: flags in scratch that survived a call would change the next."""
    import torch
    from orbslam2_amd import api
    ctx = context(api)
    st = torch.cuda.Stream()
    for name, (kf1, kf2) in S.scenes().items():
        k1, k2 = _Kf(api, kf1), _Kf(api, kf2)
        torch.cuda.synchronize()
        for s in S.SETTINGS:
            ref, nref = S.oracle(kf1, kf2, *s)
            sref, snref = _sync(ctx, kf1, kf2, *s)
            assert snref == nref and np.array_equal(sref, ref), (name, s)
            for pairs in (True, False):
                out = _Out(k1.n)
                torch.cuda.synchronize()
                out.single(ctx, k1, k2, *s, st, pairs)
                st.synchronize()
                _check_row(out.fetch(), 0, ref, nref, pairs, (name, s, pairs))
    ctx.close()


@pytest.mark.gpu
def test_gpu_the_family_in_one_batch_call_and_as_single_calls():
    """2. Per setting the batch and the K single calls on one stream, one synchronise: every row equals the oracle and batch equals
    single bit for bit.  Then, without a host step in between: two batches with different settings (the second over the reversed
    records), a single call on the big-node scene, the reversed batch again, a one-record batch and a small single call; the flags in
    scratch are reused by all of them and must be clean."""
    import torch
    from orbslam2_amd import api
    ctx = context(api)
    st = torch.cuda.Stream()
    kf1, fam = S.family()
    K, n1 = len(fam), len(kf1["d"])
    k1, kfs = _Kf(api, kf1), [_Kf(api, kf) for kf in fam]
    fwd, rev, just_one = _rec_array(kfs), _rec_array(kfs[::-1]), _rec_array(kfs[2:3])
    max_n = max(kf.n for kf in kfs)
    refs = {s: [S.oracle(kf1, kf, *s) for kf in fam] for s in S.SETTINGS}
    for s in S.SETTINGS:
        bat, one = _Out(n1, K), _Out(n1, K)
        torch.cuda.synchronize()  # the sentinels and records are in place
        bat.batch(ctx, k1, fwd, max_n, *s, st)
        for k, kf in enumerate(kfs):
            one.single(ctx, k1, kf, *s, st, row=k)
        st.synchronize()
        got, single = bat.fetch(), one.fetch()
        for k in range(K):
            _check_row(got, k, *refs[s][k], what=(s, S.FAMILY[k]))
        assert _same(got, single), s
    s0, s1 = S.SETTINGS[0], S.SETTINGS[1]
    b1, b2 = S.big_node()
    kb1, kb2 = _Kf(api, b1), _Kf(api, b2)
    a, b, c, d, e, f = _Out(n1, K), _Out(n1, K), _Out(kb1.n), _Out(n1, K), _Out(n1), _Out(n1)
    torch.cuda.synchronize()
    a.batch(ctx, k1, fwd, max_n, *s0, st)
    b.batch(ctx, k1, rev, max_n, *s1, st)
    c.single(ctx, kb1, kb2, *s0, st)
    d.batch(ctx, k1, rev, max_n, *s0, st)
    e.batch(ctx, k1, just_one, kfs[2].n, *s1, st)
    f.single(ctx, k1, kfs[2], *s1, st)
    st.synchronize()
    ga, gb, gd = a.fetch(), b.fetch(), d.fetch()
    for k in range(K):
        _check_row(ga, k, *refs[s0][k], what=("a", S.FAMILY[k]))
        _check_row(gb, K - 1 - k, *refs[s1][k], what=("b", S.FAMILY[k]))
    assert _same([g[::-1] for g in gd], ga)  # the reversed record array gives the reversed rows
    _check_row(c.fetch(), 0, *S.oracle(b1, b2, *s0), what="big node")
    gf = f.fetch()
    _check_row(gf, 0, *refs[s1][2], what="single")
    assert _same(e.fetch(), gf)  # n_kfs == 1 equals the single call
    ctx.close()


@pytest.mark.gpu
def test_gpu_more_candidates_than_a_wave_has_lanes():
    """3. 70 candidates of 200 keypoints: every row equals the oracle."""
    import torch
    from orbslam2_amd import api
    ctx = context(api)
    st = torch.cuda.Stream()
    kf1, cands = S.kf1_of_family(), S.small_candidates(70)
    k1, kfs = _Kf(api, kf1), [_Kf(api, kf) for kf in cands]
    out, d_recs = _Out(k1.n, 70), _rec_array(kfs)
    torch.cuda.synchronize()
    out.batch(ctx, k1, d_recs, 200, 0.75, True, st)
    st.synchronize()
    got = out.fetch()
    counts = []
    for k, kf in enumerate(cands):
        ref, nref = S.oracle(kf1, kf, 0.75, True)
        assert nref > 25, (k, nref)
        counts.append(nref)
        _check_row(got, k, ref, nref, what=k)
    print("70 candidates: nref %d .. %d" % (min(counts), max(counts)))
    ctx.close()


@pytest.mark.gpu
def test_gpu_empty_shapes():
    """4."""
    import torch
    from orbslam2_amd import api
    ctx = context(api)
    st = torch.cuda.Stream()
    kf1, fam = S.family()
    n1 = len(kf1["d"])
    k1, tiny, sparse = _Kf(api, kf1), _Kf(api, fam[2]), _Kf(api, fam[1])
    recs = _rec_array([tiny, sparse])
    s0 = S.SETTINGS[0]
    # n_kfs == 0: OK, nothing queued (with and without a record array)
    out = _Out(n1, 2)
    torch.cuda.synchronize()
    out.batch(ctx, k1, None, 800, *s0, st, n_kfs=0)
    out.batch(ctx, k1, recs, 800, *s0, st, n_kfs=0)
    st.synchronize()
    assert out.untouched()
    # kf1->n == 0: every row count 0 and status 0, nothing else written
    empty1 = _Kf(api, kf1, nnodes=0, n=0)
    out, one = _Out(0, 2), _Out(0)
    torch.cuda.synchronize()
    out.batch(ctx, empty1, recs, 800, *s0, st)
    one.single(ctx, empty1, tiny, *s0, st)
    st.synchronize()
    for o in (out, one):
        m, p, nm, status = o.fetch()
        assert (nm == 0).all() and (status == 0).all()
        assert o.g[0].untouched() and o.g[1].untouched()
    # kf1 without nodes; a candidate record of all NULLs and zeros; a candidate with no node in common
    nothing = np.full(n1, -1, np.int32)
    null_rec = api.BowKeyframe(None, None, None, None, None, None, None, 0, 0)
    other = _Kf(api, fam[1], nodes=(fam[1]["fv"][0] + 100000).astype(np.uint32))
    cases = {
        "kf1->nnodes == 0": (_Kf(api, kf1, nnodes=0), [tiny, sparse], [(nothing, 0)] * 2),
        "a record of NULLs and zeros": (k1, [tiny, null_rec, sparse], [S.oracle(kf1, fam[2], *s0), (nothing, 0), S.oracle(kf1, fam[1], *s0)]),
        "no node in common": (k1, [other, tiny], [(nothing, 0), S.oracle(kf1, fam[2], *s0)]),
    }
    for what, (q, kfs, refs) in cases.items():
        out, d_recs = _Out(n1, len(kfs)), _rec_array(kfs)
        torch.cuda.synchronize()
        out.batch(ctx, q, d_recs, 800, *s0, st)
        st.synchronize()
        got = out.fetch()
        for k, (ref, nref) in enumerate(refs):
            _check_row(got, k, ref, nref, what=what)
    for what, (q, c) in {"single, kf1 without nodes": (_Kf(api, kf1, nnodes=0), tiny), "single, NULL kf2": (k1, null_rec), "single, no node in common": (k1, other)}.items():
        out = _Out(n1)
        torch.cuda.synchronize()
        out.single(ctx, q, c, *s0, st)
        st.synchronize()
        _check_row(out.fetch(), 0, nothing, 0, what=what)
    ctx.close()


@pytest.mark.gpu
def test_gpu_what_the_host_refuses_queues_nothing():
    """5. Each refusal raises and leaves the outputs untouched; a clean call afterwards works."""
    import torch
    from orbslam2_amd import api
    ctx = context(api)
    st = torch.cuda.Stream()
    kf1, fam = S.family()
    n1 = len(kf1["d"])
    k1, tiny = _Kf(api, kf1), _Kf(api, fam[2])
    recs = _rec_array([tiny])
    s0 = S.SETTINGS[0]
    out = _Out(n1)
    torch.cuda.synchronize()
    null_arrays = [api.BowKeyframe(*[None if j == i else k1.t[name][1] for j, name in enumerate(_Kf.ORDER)], None, k1.nnodes, k1.n) for i in range(6)]
    bad_records = [None, _Kf(api, kf1, n=-1).rec, _Kf(api, kf1, nnodes=-1).rec, _Kf(api, kf1, n=65536).rec] + null_arrays
    for bad in bad_records:
        with pytest.raises(api.OrbfeError):
            out.batch(ctx, bad, recs, 40, *s0, st)
        with pytest.raises(api.OrbfeError):
            out.single(ctx, bad, tiny, *s0, st)
        with pytest.raises(api.OrbfeError):
            out.single(ctx, k1, bad, *s0, st)  # the single call checks kf2 in the same way
    for kw in (dict(n_kfs=-1), dict(n_kfs=65536), dict(max_kf_n=-1), dict(max_kf_n=65536), dict(d_recs=None)):
        with pytest.raises(api.OrbfeError):
            out.batch(ctx, k1, kw.get("d_recs", recs), kw.get("max_kf_n", 40), *s0, st, n_kfs=kw.get("n_kfs"))
    for k in (0, 2, 3):  # a NULL required output
        p = [out.ptr(0), out.ptr(1), out.ptr(2), out.ptr(3)]
        p[k] = 0
        with pytest.raises(api.OrbfeError):
            ctx.enqueue_search_by_bow_kf_batch(k1.rec, recs.data_ptr(), 1, 40, *s0, p[0], p[2], p[3], d_pairs=p[1], stream=st.cuda_stream)
        with pytest.raises(api.OrbfeError):
            ctx.enqueue_search_by_bow_kf(k1.rec, tiny.rec, *s0, p[0], p[2], p[3], d_pairs=p[1], stream=st.cuda_stream)
    st.synchronize()
    assert out.untouched()
    out.batch(ctx, k1, recs, 40, *s0, st)  # the context still works
    st.synchronize()
    _check_row(out.fetch(), 0, *S.oracle(kf1, fam[2], *s0), what="after the refusals")
    ctx.close()


@pytest.mark.gpu
def test_gpu_what_only_the_device_sees_is_reported_in_the_row_and_changes_no_other_row():
    """6. Three candidates (perturbed, tiny, sparse), one fault at a time: its row reports ORBFE_ERR_INVALID (a fault of KF1: every
    row that meets it), the other rows are exact, no guard cell is written, and a clean call follows each."""
    import torch
    from orbslam2_amd import api
    ctx = context(api)
    st = torch.cuda.Stream()
    kf1, fam = S.family()
    n1 = len(kf1["d"])
    cands = [fam[0], fam[2], fam[1]]
    s0 = S.SETTINGS[0]
    refs = [S.oracle(kf1, kf, *s0) for kf in cands]
    k1, kfs = _Kf(api, kf1), [_Kf(api, kf) for kf in cands]
    clean = _rec_array(kfs)
    max_n = max(kf.n for kf in kfs)
    pert = cands[0]
    fv1, fv2 = kf1["fv"], pert["fv"]
    shared1 = np.nonzero(np.isin(fv1[0], fv2[0]))[0]
    shared2 = np.nonzero(np.isin(fv2[0], fv1[0]))[0]
    # a KF2 keypoint of `perturbed` that survives the rotation cut, matched by a KF1 keypoint of angle < 20: angle1 - 400 + 360 < -20 rounds to bin -1
    matched2 = int(refs[0][0][np.nonzero((refs[0][0] >= 0) & (kf1["ang"] < 20))[0][0]])
    swap1 = fv1[0].copy(); swap1[[5, 6]] = swap1[[6, 5]]
    swap2 = fv2[0].copy(); swap2[[5, 6]] = swap2[[6, 5]]

    def with_record0(**kw):
        return k1, [_Kf(api, pert, **kw)] + kfs[1:], max_n, (0,)

    cases = {
        "n > max_kf_n in one record": (k1, kfs, 1000, (0,)),
        "nnodes = -1": with_record0(nnodes=-1),
        "two node ids swapped on the KF1 side": (_Kf(api, kf1, nodes=swap1), kfs, max_n, (0, 1, 2)),
        "two node ids swapped on a candidate": with_record0(nodes=swap2),
        "a descending CSR offset": with_record0(off=_edit(fv2[1], 7, fv2[1][6] - 1)),
        "an offset beyond n": with_record0(off=_edit(fv2[1], -1, len(pert["d"]) + 1)),
        "a KF2 feature index equal to n, in a shared node": with_record0(feat=_edit(fv2[2], fv2[1][shared2[3]], len(pert["d"]))),
        "a KF1 feature index equal to n, in a shared node": (_Kf(api, kf1, feat=_edit(fv1[2], fv1[1][shared1[3]], n1)), kfs, max_n, (0,)),
        "an angle of 400 on a matched keypoint": with_record0(angle=_edit(pert["ang"], matched2, 400.0)),
    }
    assert np.isin(fv1[0][shared1[3]], cands[0]["fv"][0]) and len(cands[0]["d"]) > 1000 >= len(cands[2]["d"])
    for what, (q, recs, bound, refused) in cases.items():
        out, again, d_recs = _Out(n1, 3), _Out(n1, 3), _rec_array(recs)
        torch.cuda.synchronize()
        out.batch(ctx, q, d_recs, bound, *s0, st)
        again.batch(ctx, k1, clean, max_n, *s0, st)
        st.synchronize()
        got = out.fetch()  # and the guards
        for k in range(3):
            if k in refused:
                assert got[3][k][0] == api.ERR_INVALID, (what, k, int(got[3][k][0]))
            elif q is k1:
                _check_row(got, k, *refs[k], what=what)
        if what in ("n > max_kf_n in one record", "nnodes = -1"):  # searched as a keyframe without nodes
            assert got[2][0][0] == 0 and (got[0][0] == -1).all(), what
        g = again.fetch()
        for k in range(3):
            _check_row(g, k, *refs[k], what=("after", what))
    ctx.close()


@pytest.mark.gpu
def test_gpu_two_batches_with_a_patch_of_valid1_on_the_stream_in_between():
    """7. Batch, a torch op on the stream that clears `valid` of the KF1 keypoints candidate 0 matched (the caller hands those map
    points on), a second batch, one synchronise: both equal the oracle run with the same patch."""
    import torch
    from orbslam2_amd import api
    ctx = context(api)
    st = torch.cuda.Stream()
    kf1, fam = S.family()
    n1 = len(kf1["d"])
    cands = fam[:3]
    k1, kfs = _Kf(api, kf1), [_Kf(api, kf) for kf in cands]
    d_recs = _rec_array(kfs)
    max_n = max(kf.n for kf in kfs)
    s0 = S.SETTINGS[0]
    first, second = _Out(n1, 3), _Out(n1, 3)
    valid1 = k1.t["valid"][0].view(torch.int32)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        first.batch(ctx, k1, d_recs, max_n, *s0, st)
        row0 = first.g[0].view[:n1]
        valid1[:n1] = torch.where(row0 >= 0, torch.zeros_like(row0), valid1[:n1])
        second.batch(ctx, k1, d_recs, max_n, *s0, st)
    st.synchronize()
    g1, g2 = first.fetch(), second.fetch()
    patched = kf1["valid"].copy()
    for k, kf in enumerate(cands):
        _check_row(g1, k, *S.oracle(kf1, kf, *s0), what=("first", k))
    patched[S.oracle(kf1, cands[0], *s0)[0] >= 0] = 0
    assert patched.sum() < kf1["valid"].sum() - 300
    for k, kf in enumerate(cands):
        ref, nref = S.oracle(kf1, kf, *s0, valid1=patched)
        _check_row(g2, k, ref, nref, what=("second", k))
    assert g2[2][0][0] < g1[2][0][0] // 4  # candidate 0 finds only what its earlier matches had blocked
    assert np.array_equal(valid1[:n1].cpu().numpy(), patched)
    ctx.close()
