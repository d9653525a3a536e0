"""SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist) on the device-resident frame, for one candidate keyframe and
for all candidates of a relocalisation in one call (orbfe_enqueue_search_by_projection_kf, orbfe_enqueue_search_by_projection_kf_batch;
orbslam2_amd/csrc/orbfe_match_device.hip).  Every comparison of matches is exact.

The expectation (_expect) is the CPU oracle's search_by_projection_kf, unchanged, behind the two steps that the entry points add
(include/orbfe.h): found[i] = some keypoint holds keyframe point i at entry (only with exclude_held), then the outlier clear of
cur_point; the oracle is called with kf_valid & ~found and has_point = cur_point >= 0.

cur_point is made realistic in two passes (_held): the oracle at (10, 100, rotation check) with nothing held, a random 50-60 % of
its matches kept as cur_point, outlier drawn with p = 0.25-0.3.  The first CPU test shows that on these inputs the exclusion, the
outlier clear, the blocking inside a call and the re-scan beyond the four-key prefix each change the answer, so the exact
comparisons of the GPU tests decide them.

GPU: synthetic frames become image slot 0 by test_gpu_matcher_census._inject_unfetched -- test_matchers_device._inject for an
extraction call of which nothing is fetched, which the SYNCHRONOUS resident view needs too (a fetched count would make it refuse
the injected one as stale); the real-frame test uses the extraction's own keypoints.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import matcher_census as MC
from tests import test_matchers as TM
from tests import test_matchers_device as TD
from tests.device_arrays import BEYOND, HAS_UNTOUCHED, UNTOUCHED, XW_UNTOUCHED, Guarded, context, device_buffers, raw, upload, upload_records

W, H, NL, LOG_SF, CAM = TM.W, TM.H, TM.NL, TM.LOG_SF, TM.CAM
NEW = ["orbfe_enqueue_search_by_projection_kf", "orbfe_enqueue_search_by_projection_kf_batch"]
ERR_INVALID, ERR_CAPACITY = -1, -4
PLAIN = ("track_30", "among", "retreat", "sideways", "tie", "tie_wide", "overflow")  # every census input that lists `kf`
STAGES = ((10.0, 100, False), (3.0, 64, True))  # the two call sites of Relocalization (src/Tracking.cc:1552, :1566)


# ------------------------------------------------------------------ inputs and expectation (CPU)
def _frame(s):
    return dict(k=s["k"], d=s["d"], ur=s["ur"], bounds=s["bounds"], sf=s["sf"], grid=O.Grid(s["k"], *s["bounds"]))


def _rec(s, th, od, idx=None, T=None, valid=None):
    """One candidate keyframe: the scene's map points (or the rows idx of them) seen from T."""
    idx = np.arange(len(s["pos"])) if idx is None else np.asarray(idx)
    v = s["valid"] if valid is None else valid
    return dict(T=np.ascontiguousarray(s["T_cur"] if T is None else T, np.float32), pos=s["pos"][idx], desc=s["desc"][idx],
                valid=np.ascontiguousarray(v[idx], np.int32), angle=s["angle"][idx], max_d=s["max_d"][idx], min_d=s["min_d"][idx], th=float(th), od=int(od))


def _oracle(fr, rec, valid, has, th, od, ori):
    nk = len(fr["k"])
    if len(valid) == 0:
        return np.full(nk, -1, np.int32), 0
    return O.search_by_projection_kf(fr["grid"], fr["d"], fr["sf"], CAM, rec["T"], LOG_SF, NL, rec["pos"], rec["desc"], valid, rec["angle"], rec["max_d"],
                                     rec["min_d"], has, th, od, ori)


def _expect(fr, rec, cur_point, outlier, exclude_held, ori, th=None, od=None, exclusion=True, clear=True):
    """What the entry points write for one candidate.  exclusion / clear = False: the two wrong variants of the first CPU test."""
    n = len(rec["valid"])
    cp = np.asarray(cur_point, np.int32).copy()
    bad = (cp < -1) | (cp >= n)
    cp[bad] = -1
    found = np.zeros(n, bool)
    if exclude_held and exclusion:
        found[cp[cp >= 0]] = True
    if outlier is not None and clear:
        cp[np.asarray(outlier) != 0] = -1
    match, nm = _oracle(fr, rec, (rec["valid"].astype(bool) & ~found).astype(np.int32), (cp >= 0).astype(np.uint8), rec["th"] if th is None else th,
                        rec["od"] if od is None else od, ori)
    out = np.where(match >= 0, match, cp).astype(np.int32)
    return dict(match=match, nm=nm, cur_point=out, has=(out >= 0).astype(np.uint8), status=ERR_INVALID if bad.any() else 0)


def _held(fr, rec, seed, keep=0.55, p_out=0.28):
    """The two-pass construction of the module docstring: (cur_point, outlier)."""
    rng = np.random.default_rng(seed)
    nk = len(fr["k"])
    first, _ = _oracle(fr, rec, rec["valid"], np.zeros(nk, np.uint8), 10.0, 100, True)
    cp = np.where((first >= 0) & (rng.random(nk) < keep), first, -1).astype(np.int32)
    return cp, (rng.random(nk) < p_out).astype(np.uint8)


_CACHE = {}


def _scene(name):
    """A census input, the 1500-point tracking scene ("track_1500") or the prefix scene ("prefix"), built once."""
    if name in _CACHE:
        return _CACHE[name]
    if name == "track_1500":
        s = MC._existing_tracking(31, n_last=1500)
    elif name == "prefix":
        # every map point 10 times, its keypoint 8 times: under the keyframe rule every accepted keypoint is closed, so copy j of a
        # point takes the j-th best of its cluster and copies 5 .. 8 find all four keys of their prefix taken.  1500 queries: more
        # than the 1024 the resolve kernel stages at a time
        s = dict(TD._prefix_scene())
        T = s["T_cur"].astype(np.float64)
        dist = np.linalg.norm(s["pos"].astype(np.float64) + (T[:, :3].T @ T[:, 3]), axis=1)  # |P - Ow|, Ow = -R^T t
        s["max_d"] = (0.97 * dist * 1.2 ** s["octave"]).astype(np.float32)
        s["min_d"] = (s["max_d"] / np.float32(1.2 ** 7) / 2).astype(np.float32)
        s["repeat"] = np.tile(np.arange(10), len(s["pos"]) // 10)  # np.repeat(x, 10): row i is copy i % 10 of point i // 10
        assert len(s["k"]) == 1300 and len(s["pos"]) == 1500
    else:
        s = MC.build(name)
    _CACHE[name] = s
    return s


def _kf_params(name):
    return MC.INPUTS[name][1]["kf"] if name in MC.INPUTS else (10.0, 100, True)


def _family(name):
    """The candidates of the batch tests on one frame: (frame, [(what, record, cur_point, outlier)]), at least seven records that
    no two rows of outputs agree on."""
    key = ("family", name)
    if key in _CACHE:
        return _CACHE[key]
    s = _scene(name)
    fr = _frame(s)
    th, od, _ = _kf_params(name)
    n = len(s["pos"])
    rng = np.random.default_rng(77)
    T2 = s["T_cur"].copy(); T2[:, 3] += np.array([0.03, -0.02, 0.05], np.float32)
    sub60 = np.sort(rng.permutation(n)[: int(0.6 * n)])
    sub40 = np.sort(rng.permutation(n)[:40])
    members = [("full", _rec(s, th, od), 1, 0.28), ("perturbed pose", _rec(s, th, od, T=T2), 2, 0.28), ("60 % at (3, 64)", _rec(s, 3.0, 64, sub60), 3, 0.28),
               ("40 points", _rec(s, th, od, sub40), 4, 0.28), ("th 15, heavy outlier", _rec(s, 15.0, od), 5, 0.6)]
    out = [(what, rec) + _held(fr, rec, seed, p_out=p) for what, rec, seed, p in members]
    out.append(("all invalid", _rec(s, th, od, valid=np.zeros_like(s["valid"])), out[0][2].copy(), out[0][3].copy()))  # holds the full keyframe's points
    empty = _rec(s, th, od, np.zeros(0, np.int64))
    out.append(("n == 0", empty, np.full(len(fr["k"]), -1, np.int32), out[1][3].copy()))
    _CACHE[key] = (fr, out)
    return _CACHE[key]


# ------------------------------------------------------------------ CPU
def test_the_library_exports_both_calls_and_the_candidate_record():
    from orbslam2_amd import api
    L = api.load()
    for name in NEW:
        assert name in api.EXPORTS
        fn = getattr(L, name)  # AttributeError: the symbol is not exported
        args = [0 if t is C.c_int else 0.0 if t is C.c_float else None for t in fn.argtypes]
        assert fn(*args) == api.ERR_INVALID, name
    assert callable(api.Context.enqueue_search_by_projection_kf) and callable(api.Context.enqueue_search_by_projection_kf_batch)
    assert C.sizeof(api.RelocCandidate) == 88
    assert api.RelocCandidate.n.offset == 72 and api.RelocCandidate.reserved.offset == 84


def test_the_inputs_tell_the_behaviours_apart():
    """Oracle only.  On the two-pass inputs: dropping the `found` exclusion changes the row on every chained scene; dropping the
    outlier clear changes it on `overflow` (the other scenes are too sparse for a freed keypoint to be taken by another point, which is
    why `overflow` is in every chained test); without the blocking inside a call several queries of `overflow` claim one keypoint
    (the oracle run one query at a time); on the prefix scene queries with repeat index >= 5 take keypoints beyond their
    four-key prefix; any two rows of the batch families differ.  Figures of this construction (printed): 28 - 65 entries differ without
    the exclusion (overflow 2 - 3), 2 - 3 without the outlier clear on overflow and none elsewhere, 23 of overflow's 25 matched keypoints
    are claimed by more than one query alone, the prefix scene gives 532 and 585 matches."""
    for name in ("tie", "retreat", "sideways", "track_30", "overflow", "track_1500"):
        s = _scene(name)
        fr = _frame(s)
        th, od, _ = _kf_params(name)
        rec = _rec(s, th, od)
        cp, outl = _held(fr, rec, 5)
        assert 0.5 * (cp >= 0).sum() > ((cp >= 0) & (outl != 0)).sum() > 0
        for th_, od_, ori in STAGES:
            ref = _expect(fr, rec, cp, outl, 1, ori, th_, od_)
            no_excl = _expect(fr, rec, cp, outl, 1, ori, th_, od_, exclusion=False)
            no_clear = _expect(fr, rec, cp, outl, 1, ori, th_, od_, clear=False)
            d_excl, d_clear = int((ref["match"] != no_excl["match"]).sum()), int((ref["match"] != no_clear["match"]).sum())
            print("%s %s: %d matches; without the exclusion %d entries differ, without the outlier clear %d" % (name, (th_, od_, ori), ref["nm"], d_excl, d_clear))
            if (th_, od_) == (10.0, 100):
                assert d_excl > 0, name
                assert (d_clear > 0) == (name == "overflow"), (name, d_clear)
    # blocking inside a call
    for name in ("overflow", "tie", "retreat"):
        s = _scene(name)
        fr = _frame(s)
        th, od, ori = _kf_params(name)
        rec = _rec(s, th, od)
        none = np.zeros(len(fr["k"]), np.uint8)
        full, _ = _oracle(fr, rec, rec["valid"], none, th, od, False)
        claims = np.zeros(len(fr["k"]), np.int64)
        for i in np.nonzero(rec["valid"])[0]:
            one = np.zeros_like(rec["valid"]); one[i] = 1
            m, nm = _oracle(fr, rec, one, none, th, od, False)
            claims += m >= 0
        matched = full >= 0
        print("%s: %d matched keypoints, %d of them claimed by more than one query alone" % (name, matched.sum(), (claims[matched] > 1).sum()))
        assert ((claims[matched] > 1).sum() > 0) == (name == "overflow"), name
    # prefix exhaustion under the keyframe rule
    s = _scene("prefix")
    fr = _frame(s)
    cluster = np.arange(len(s["k"]) - 8 * s["n_clusters"], len(s["k"]))
    assert 8 * s["n_clusters"] == 480
    for (th, od, ori), expect in (((7.0, 100, True), 532), ((3.0, 64, False), 585)):  # the oracle's counts on this construction, pinned
        rec = _rec(s, th, od)
        m, nm = _oracle(fr, rec, rec["valid"], np.zeros(len(fr["k"]), np.uint8), th, od, ori)
        takers = m[cluster][m[cluster] >= 0]
        hist = np.bincount(s["repeat"][takers], minlength=10)
        print("prefix %s: %d matches, %d of 480 cluster keypoints matched, repeat-index histogram of their queries %s" % ((th, od, ori), nm, len(takers), hist.tolist()))
        assert nm == expect and len(takers) == 480  # every cluster keypoint is matched
        assert hist[5:].sum() > 0  # a query with repeat index >= 5 has at least five better keys taken: beyond the prefix of four
    # the batch families
    for name in ("overflow", "track_1500"):
        fr, fam = _family(name)
        assert len(fam) >= 6
        for ori in (True, False):
            rows = []
            for what, rec, cp, outl in fam:
                e = _expect(fr, rec, cp, outl, 1, ori)
                rows.append(np.concatenate([e["match"], e["cur_point"]]))
            print("%s ori %d: matches per row %s" % (name, ori, [int((r[: len(fr["k"])] >= 0).sum()) for r in rows]))
            for i in range(len(rows)):
                for j in range(i):
                    assert (rows[i] != rows[j]).any(), (name, fam[i][0], fam[j][0])


# ------------------------------------------------------------------ helpers (GPU)
def _inject(ctx, fr, st):
    from tests import test_gpu_matcher_census as TG
    TG._inject_unfetched(ctx, fr["k"], fr["d"], fr["ur"], st)


class _Cand:
    """One candidate's arrays in HBM.  cur_point / outlier span the keypoint capacity; at and beyond the frame's count they hold what
    must never be read as a keypoint's entry (BEYOND, 1)."""

    def __init__(self, rec, cur_point, outlier, cap, T=None):
        import torch
        self.rec, self.n, nk = rec, len(rec["valid"]), len(cur_point)
        self.T = upload(rec["T"])[0] if T is None else T
        self.keep = [upload(np.ascontiguousarray(x, t))[0] for x, t in ((rec["pos"], np.float32), (rec["desc"], np.uint8), (rec["valid"], np.int32),
                                                                      (rec["angle"], np.float32), (rec["max_d"], np.float32), (rec["min_d"], np.float32))]
        cp = np.full(cap, BEYOND, np.int32); cp[:nk] = cur_point
        self.cur_point = upload(cp)[0]
        self.outlier = None
        if outlier is not None:
            o = np.ones(cap, np.uint8); o[:nk] = outlier
            self.outlier = upload(o)[0]
        self.cp_in = np.asarray(cur_point, np.int32).copy()
        torch.cuda.synchronize()

    def ptrs(self):
        return [self.T.data_ptr()] + [t.data_ptr() if t.numel() else 0 for t in self.keep] + [self.cur_point.data_ptr(),
                                                                                             0 if self.outlier is None else self.outlier.data_ptr()]

    def record(self, api, **over):
        p = self.ptrs()
        f = dict(zip(("Tcw", "pos", "desc", "valid", "angle", "max_distance", "min_distance", "cur_point", "outlier"), [x or None for x in p]))
        f.update(n=self.n, th=self.rec["th"], orb_dist=self.rec["od"], reserved=0)
        f.update(over)
        return api.RelocCandidate(**f)


class _Rows:
    """K rows of outputs between guards, every cell holding a sentinel; filled by one batch call or row by row by the single call."""

    def __init__(self, cap, K, has_fill=HAS_UNTOUCHED):
        import torch
        self.cap, self.K = cap, K
        self.match, self.nm, self.status = Guarded.cells(K * cap), Guarded.cells(K), Guarded.cells(K)
        self.has = Guarded(np.full(K * cap, has_fill, np.uint8))
        self.Xw = Guarded(np.full(K * cap * 3, XW_UNTOUCHED, np.float32))
        torch.cuda.synchronize()

    def single(self, ctx, c, cand, bounds, ori, exclude, st):
        p = cand.ptrs()
        ctx.enqueue_search_by_projection_kf(0, bounds, p[0], cand.n, p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], cand.rec["th"], cand.rec["od"], ori, exclude,
                                            self.match.ptr + 4 * c * self.cap, self.nm.ptr + 4 * c, self.status.ptr + 4 * c, self.has.ptr + c * self.cap,
                                            self.Xw.ptr + 12 * c * self.cap, st.cuda_stream)

    def batch(self, ctx, d_recs, K, max_n, bounds, ori, exclude, st):
        ctx.enqueue_search_by_projection_kf_batch(0, bounds, d_recs.data_ptr(), K, max_n, ori, exclude, self.match.ptr, self.nm.ptr,
                                                  self.status.ptr, self.has.ptr, self.Xw.ptr, st.cuda_stream)

    def fetch(self, cands):
        K, cap = self.K, self.cap
        return dict(match=self.match.fetch().reshape(K, cap), nm=self.nm.fetch(), status=self.status.fetch(), has=self.has.fetch().reshape(K, cap),
                    Xw=self.Xw.fetch().reshape(K, cap, 3), cur_point=np.stack([c.cur_point.cpu().numpy() for c in cands]))


def _check_row(got, c, nk, cand, exp, what, has_fill=HAS_UNTOUCHED):
    """Row c after the stream was synchronised: exactly the expectation, nothing read or written at or beyond the keypoint count."""
    assert int(got["status"][c]) == exp["status"], (what, int(got["status"][c]))
    if exp["status"] != 0:
        return
    assert int(got["nm"][c]) == exp["nm"], (what, int(got["nm"][c]), exp["nm"])
    bad = np.nonzero(got["match"][c][:nk] != exp["match"])[0]
    assert bad.size == 0, "%s: differ at %s: HIP %s, oracle %s" % (what, bad[:8].tolist(), got["match"][c][bad[:8]].tolist(), exp["match"][bad[:8]].tolist())
    assert (got["match"][c][nk:] == UNTOUCHED).all(), what
    assert np.array_equal(got["cur_point"][c][:nk], exp["cur_point"]) and (got["cur_point"][c][nk:] == BEYOND).all(), what
    assert np.array_equal(got["has"][c][:nk], exp["has"]) and (got["has"][c][nk:] == has_fill).all(), what
    h = exp["has"] != 0
    Xw = got["Xw"][c]
    assert np.array_equal(Xw[:nk][h], cand.rec["pos"][exp["cur_point"][h]]), what  # held before the call and newly matched alike
    assert (Xw[:nk][~h] == XW_UNTOUCHED).all() and (Xw[nk:] == XW_UNTOUCHED).all(), what


def _sync_kf(ctx, fr, rec, cur_point, outlier, exclude, ori):
    """The expectation's steps around the SYNCHRONOUS entry point on the resident view of slot 0: (matches, count)."""
    n = len(rec["valid"])
    cp = np.asarray(cur_point, np.int32).copy()
    found = np.zeros(n, bool)
    if exclude:
        found[cp[cp >= 0]] = True
    if outlier is not None:
        cp[outlier != 0] = -1
    view = ctx._view(fr["k"], None, fr["d"], fr["bounds"], device_slot=0)
    return ctx.search_by_projection_kf(view, rec["T"][:3], rec["pos"], rec["desc"], (rec["valid"].astype(bool) & ~found).astype(np.int32), rec["angle"],
                                       rec["max_d"], rec["min_d"], (cp >= 0).astype(np.uint8), rec["th"], rec["od"], ori)


def _ctx_for(api, fr, **kw):
    ctx = context(api, nfeatures=max(2000, len(fr["k"]) + 200), **kw)
    assert ctx.capacity >= len(fr["k"])
    return ctx


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", PLAIN)
def test_gpu_plain_mode_equals_the_oracle_and_the_synchronous_resident_call(name):
    """exclude_held = 0, no outlier array, cur_point = where(has, 0, -1): the synchronous entry point's contract, on every census
    input that lists `kf` with its own parameters (tie_wide: keypoint indices above 32768); two calls, the second on the cached grid."""
    import torch
    from orbslam2_amd import api
    s = _scene(name)
    fr = _frame(s)
    th, od, ori = _kf_params(name)
    rec = _rec(s, th, od)
    nk = len(fr["k"])
    cp = np.where(s["has"] != 0, 0, -1).astype(np.int32)
    exp = _expect(fr, rec, cp, None, 0, ori)
    ref = MC.oracle_run("kf", s, (th, od, ori))
    assert exp["nm"] == ref[1] and np.array_equal(exp["match"], ref[0]) and exp["nm"] > 0
    ctx = _ctx_for(api, fr)
    st = torch.cuda.Stream()
    _inject(ctx, fr, st)
    got, ngot = _sync_kf(ctx, fr, rec, cp, None, 0, ori)
    assert ngot == exp["nm"] and np.array_equal(got, exp["match"]), name
    for rep in range(2):
        cand = _Cand(rec, cp, None, ctx.capacity)
        rows = _Rows(ctx.capacity, 1)
        rows.single(ctx, 0, cand, fr["bounds"], ori, 0, st)
        st.synchronize()
        _check_row(rows.fetch([cand]), 0, nk, cand, exp, "%s, call %d" % (name, rep))
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["overflow", "tie", "retreat", "track_1500"])
def test_gpu_chained_mode_excludes_the_held_points_and_clears_the_outliers(name):
    """The two-pass inputs with exclude_held = 1 and an outlier array, at both stages of Relocalization."""
    import torch
    from orbslam2_amd import api
    s = _scene(name)
    fr = _frame(s)
    nk = len(fr["k"])
    ctx = _ctx_for(api, fr)
    st = torch.cuda.Stream()
    _inject(ctx, fr, st)
    for th, od, ori in STAGES:
        rec = _rec(s, th, od)
        cp, outl = _held(fr, rec, 5)
        exp = _expect(fr, rec, cp, outl, 1, ori)
        assert exp["nm"] > 0 and exp["status"] == 0
        got, ngot = _sync_kf(ctx, fr, rec, cp, outl, 1, ori)
        assert ngot == exp["nm"] and np.array_equal(got, exp["match"]), (name, th)
        cand = _Cand(rec, cp, outl, ctx.capacity)
        rows = _Rows(ctx.capacity, 1)
        rows.single(ctx, 0, cand, fr["bounds"], ori, 1, st)
        st.synchronize()
        _check_row(rows.fetch([cand]), 0, nk, cand, exp, "%s at %s" % (name, (th, od, ori)))
    ctx.close()


@pytest.mark.gpu
def test_gpu_prefix_runs_out_across_the_chunk_and_a_second_call_chains_on_cur_point():
    """The prefix scene (1500 queries: two chunks of the resolve kernel; copies 5 .. 8 of a point re-scan their window), then a second
    call on the same context whose input is the cur_point the first call left in HBM, with an outlier array."""
    import torch
    from orbslam2_amd import api
    s = _scene("prefix")
    fr = _frame(s)
    nk = len(fr["k"])
    ctx = _ctx_for(api, fr)
    st = torch.cuda.Stream()
    _inject(ctx, fr, st)
    outl = (np.random.default_rng(8).random(nk) < 0.28).astype(np.uint8)
    for (th, od, ori), n1 in (((7.0, 100, True), 532), ((3.0, 64, False), 585)):
        rec = _rec(s, th, od)
        cp0 = np.full(nk, -1, np.int32)
        exp1 = _expect(fr, rec, cp0, None, 1, ori)
        assert exp1["nm"] == n1
        exp2 = _expect(fr, rec, exp1["cur_point"], outl, 1, ori)
        assert exp2["nm"] > 20  # keypoints freed by the outlier clear are taken by the copies that found nothing
        cand = _Cand(rec, cp0, None, ctx.capacity)
        rows1, rows2 = _Rows(ctx.capacity, 1), _Rows(ctx.capacity, 1)
        rows1.single(ctx, 0, cand, fr["bounds"], ori, 1, st)
        st.synchronize()
        _check_row(rows1.fetch([cand]), 0, nk, cand, exp1, "first call at %s" % ((th, od, ori),))
        o = np.ones(ctx.capacity, np.uint8); o[:nk] = outl
        cand.outlier = upload(o)[0]
        torch.cuda.synchronize()
        rows2.single(ctx, 0, cand, fr["bounds"], ori, 1, st)
        st.synchronize()
        got = rows2.fetch([cand])
        _check_row(got, 0, nk, cand, exp2, "second call at %s" % ((th, od, ori),))
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["overflow", "track_1500"])
def test_gpu_batch_rows_equal_the_single_call_bit_for_bit_and_the_oracle(name):
    """Seven records per call (full keyframe, perturbed pose, a 60 % subset at (3, 64), 40 points, th 15 with heavy outliers, all invalid,
    n == 0), a second batch of another size and order back to back on the same stream before synchronising, then the single call per
    record."""
    import torch
    from orbslam2_amd import api
    fr, fam = _family(name)
    nk = len(fr["k"])
    ctx = _ctx_for(api, fr)
    cap = ctx.capacity
    st = torch.cuda.Stream()
    _inject(ctx, fr, st)
    order2 = [4, 2, 0, 3]
    a = [_Cand(rec, cp, outl, cap) for _, rec, cp, outl in fam]
    b = [_Cand(fam[i][1], fam[i][2], fam[i][3], cap) for i in order2]
    rows_a, rows_b = _Rows(cap, len(a)), _Rows(cap, len(b))
    recs_a, recs_b = upload_records([c.record(api) for c in a]), upload_records([c.record(api) for c in b])
    max_a, max_b = max(c.n for c in a), max(c.n for c in b)
    torch.cuda.synchronize()
    rows_a.batch(ctx, recs_a, len(a), max_a, fr["bounds"], True, 1, st)
    rows_b.batch(ctx, recs_b, len(b), max_b + 3, fr["bounds"], False, 1, st)  # nothing waited for in between
    st.synchronize()
    got_a, got_b = rows_a.fetch(a), rows_b.fetch(b)
    for c, (what, rec, cp, outl) in enumerate(fam):
        _check_row(got_a, c, nk, a[c], _expect(fr, rec, cp, outl, 1, True), "%s / %s, first batch" % (name, what))
    for c, i in enumerate(order2):
        what, rec, cp, outl = fam[i]
        _check_row(got_b, c, nk, b[c], _expect(fr, rec, cp, outl, 1, False), "%s / %s, second batch" % (name, what))
    assert int(got_a["nm"][:5].min()) > 0 and int(got_a["nm"][5]) == 0 and int(got_a["nm"][6]) == 0
    # the single call on every record, with fresh cur_point arrays: bit for bit what the batch wrote
    for ori, fam_idx, got in ((True, list(range(len(fam))), got_a), (False, order2, got_b)):
        cands = [_Cand(fam[i][1], fam[i][2], fam[i][3], cap) for i in fam_idx]
        rows = _Rows(cap, len(cands))
        for c, cand in enumerate(cands):
            rows.single(ctx, c, cand, fr["bounds"], ori, 1, st)
        st.synchronize()
        one = rows.fetch(cands)
        for key in ("match", "nm", "status", "has", "cur_point"):
            assert np.array_equal(one[key], got[key]), (name, ori, key)
        assert one["Xw"].tobytes() == got["Xw"].tobytes(), (name, ori)
    ctx.close()


@pytest.mark.gpu
def test_gpu_batch_refusals_on_the_device_and_on_the_host():
    """Device side: a record with n > max_n_kf, n < 0 or a NULL pos under n > 0 is reported in its status row and searched as a keyframe
    without points (none of its pointers followed: its cur_point stays as it was), its neighbours are unchanged; a cur_point entry >= n is
    reported.  Only NULL pointers and out-of-range counts are used, never a dangling pointer.  Host side: every refusal of include/orbfe.h."""
    import torch
    from orbslam2_amd import api
    fr, fam = _family("overflow")
    nk = len(fr["k"])
    ctx = _ctx_for(api, fr)
    cap = ctx.capacity
    st = torch.cuda.Stream()
    _inject(ctx, fr, st)
    cands = [_Cand(fam[i][1], fam[i][2], fam[i][3], cap) for i in (0, 1, 2, 0, 4, 3)]
    over_range = fam[3][2].copy()
    held = np.nonzero(over_range < 0)[0]
    over_range[held[0]] = fam[3][1]["valid"].size      # == n: the first index that is none
    over_range[held[1]] = -2
    cands.append(_Cand(fam[3][1], over_range, fam[3][3], cap))
    max_n = max(c.n for c in cands)
    recs = [cands[0].record(api), cands[1].record(api, n=max_n + 1), cands[2].record(api), cands[3].record(api, n=-1), cands[4].record(api),
            cands[5].record(api, pos=None), cands[6].record(api)]
    rows = _Rows(cap, len(recs))
    d_recs = upload_records(recs)
    torch.cuda.synchronize()
    rows.batch(ctx, d_recs, len(recs), max_n, fr["bounds"], True, 1, st)
    st.synchronize()
    got = rows.fetch(cands)
    for c, i in ((0, 0), (2, 2), (4, 4)):
        _check_row(got, c, nk, cands[c], _expect(fr, fam[i][1], fam[i][2], fam[i][3], 1, True), "neighbour row %d" % c)
    for c in (1, 3, 5):
        assert int(got["status"][c]) == ERR_INVALID and int(got["nm"][c]) == 0, c
        assert (got["match"][c][:nk] == -1).all() and (got["match"][c][nk:] == UNTOUCHED).all(), c
        assert (got["has"][c][:nk] == 0).all() and (got["has"][c][nk:] == HAS_UNTOUCHED).all() and (got["Xw"][c] == XW_UNTOUCHED).all(), c
        assert np.array_equal(got["cur_point"][c][:nk], cands[c].cp_in), c  # the refused record's array was not touched
    assert int(got["status"][6]) == ERR_INVALID
    assert (got["cur_point"][6][nk:] == BEYOND).all() and (got["match"][6][nk:] == UNTOUCHED).all()
    # host side
    ok = dict(d_cands=d_recs.data_ptr(), n_cands=2, max_n_kf=max_n, d_cur_match=rows.match.ptr, d_nmatches=rows.nm.ptr,
              d_status=rows.status.ptr, slot=0, bounds=fr["bounds"])

    def call(**over):
        a = dict(ok); a.update(over)
        ctx.enqueue_search_by_projection_kf_batch(a["slot"], a["bounds"], a["d_cands"], a["n_cands"], a["max_n_kf"], True, 1, a["d_cur_match"], a["d_nmatches"],
                                                  a["d_status"], 0, 0, st.cuda_stream)

    for over in (dict(d_cands=0), dict(d_cur_match=0), dict(d_nmatches=0), dict(d_status=0), dict(slot=5), dict(slot=-1), dict(n_cands=-1),
                 dict(n_cands=65536, max_n_kf=1), dict(max_n_kf=-1)):
        with pytest.raises(api.OrbfeError) as e:
            call(**over)
        assert e.value.code == api.ERR_INVALID, over
    with pytest.raises(api.OrbfeError) as e:
        call(n_cands=1025, max_n_kf=1024)  # 2^20 + 1024 scratch rows
    assert e.value.code == ERR_CAPACITY
    before = rows.fetch(cands)
    call(n_cands=0)  # ORBFE_OK, nothing queued
    call(n_cands=0, d_cands=0)
    p = cands[0].ptrs()
    for over in ((0, None), (7, 5)):  # the single call: no pose; no such slot
        args = list(p); slot = 0
        if over[1] is None:
            args[over[0]] = 0
        else:
            slot = over[1]
        with pytest.raises(api.OrbfeError) as e:
            ctx.enqueue_search_by_projection_kf(slot, fr["bounds"], args[0], cands[0].n, *args[1:9], 10.0, 100, True, 1, rows.match.ptr, rows.nm.ptr,
                                                rows.status.ptr, 0, 0, st.cuda_stream)
        assert e.value.code == api.ERR_INVALID
    st.synchronize()
    after = rows.fetch(cands)
    for key in before:
        assert np.array_equal(before[key], after[key]), key  # the refused calls queued nothing
    ctx.close()


def _real_frame(ctx, seed, distorted):
    from orbslam2_amd import synth
    left, right = synth.stereo_pair(W, H, seed=seed)
    out = ctx.stereo_frame(left, right)
    k, d, ur = out["kps_left"], out["desc_left"], out["u_right"]
    kun = ctx.fetch_keys_un(0) if distorted else k
    bounds = tuple(float(b) for b in ctx.image_bounds()) if distorted else (0.0, float(W), 0.0, float(H))
    s = TM._frame_scene(kun, d, ur, seed)
    sf = O.Extractor().scale_factors()
    dist0 = np.linalg.norm(s["pos"], axis=1).astype(np.float32)
    s["max_d"] = (dist0 * sf[s["octave"]]).astype(np.float32); s["min_d"] = (s["max_d"] / sf[NL - 1]).astype(np.float32)
    fr = dict(k=kun, d=d, ur=ur, bounds=bounds, sf=sf, grid=O.Grid(kun, *bounds))
    return fr, s


@pytest.mark.gpu
def test_gpu_real_extracted_frame_with_distortion_set():
    """A real frame (synth.stereo_pair through stereo_frame, slot 0) with distortion coefficients set: the matcher reads the keypoints
    undistorted on the device.  Plain and chained mode equal the synchronous resident call and the oracle on the undistorted keys."""
    import torch
    from orbslam2_amd import api
    ctx = context(api, nfeatures=1500)
    ctx.set_distortion([-0.28, 0.07, 2e-4, 1e-5, 0.0])
    st = torch.cuda.Stream()
    fr, s = _real_frame(ctx, 501, True)
    nk = len(fr["k"])
    rec = _rec(s, 10.0, 100)
    plain = np.where(s["has"] != 0, 0, -1).astype(np.int32)
    cp, outl = _held(fr, rec, 6)
    for what, c, o, excl, (th, od, ori) in (("plain", plain, None, 0, (10.0, 100, True)), ("chained", cp, outl, 1, (3.0, 64, True)), ("plain again", plain, None, 0, (10.0, 100, True))):
        r = dict(rec, th=th, od=od)
        exp = _expect(fr, r, c, o, excl, ori)
        assert exp["nm"] > (10 if excl else 40), what  # chained: most points are held already
        got, ngot = _sync_kf(ctx, fr, r, c, o, excl, ori)
        assert ngot == exp["nm"] and np.array_equal(got, exp["match"]), what
        cand = _Cand(r, c, o, ctx.capacity)
        rows = _Rows(ctx.capacity, 1)
        rows.single(ctx, 0, cand, fr["bounds"], ori, excl, st)
        st.synchronize()
        _check_row(rows.fetch([cand]), 0, nk, cand, exp, what)
    ctx.close()


@pytest.mark.gpu
def test_gpu_projection_then_pose_on_one_stream_without_a_host_step():
    """The batch projection of 2 candidates, then orbfe_enqueue_pose_optimization over their has_point / Xw rows (keys_un / u_right
    replicated per problem, offsets [0, cap, 2 cap]) on one stream with one synchronise: the matcher reads the very 4x4 poses that the
    optimisation then updates.  Against the same sequence through the synchronous entry points: matches exact, outlier flags and inlier
    counts equal, poses within the tolerance of tests/test_pose.py."""
    import torch
    from orbslam2_amd import api
    from tests.test_pose import POSE_ATOL
    ctx = context(api, nfeatures=1500)
    st = torch.cuda.Stream()
    fr, s = _real_frame(ctx, 701, False)
    nk, cap = len(fr["k"]), ctx.capacity
    n = len(s["pos"])
    T4 = np.eye(4, dtype=np.float32); T4[:3] = s["T_cur"]
    T4b = T4.copy(); T4b[:3, 3] += np.array([0.02, 0.01, -0.03], np.float32)
    sub = np.sort(np.random.default_rng(9).permutation(n)[: int(0.6 * n)])
    recs = [_rec(s, 10.0, 100, T=T4), _rec(s, 10.0, 100, sub, T=T4b)]
    held = [(np.full(nk, -1, np.int32), None), _held(fr, recs[1], 7)]
    # the synchronous sequence
    ref = []
    for rec, (cp, outl) in zip(recs, held):
        exp = _expect(fr, rec, cp, outl, 1, True)
        got, ngot = _sync_kf(ctx, fr, rec, cp, outl, 1, True)
        assert ngot == exp["nm"] and np.array_equal(got, exp["match"]) and exp["nm"] > 40
        Xw = np.zeros((nk, 3), np.float32); h = exp["has"] != 0
        Xw[h] = rec["pos"][exp["cur_point"][h]]
        T_host, out_host, n_host = ctx.pose_optimization(rec["T"], fr["k"], fr["ur"], exp["has"], Xw)
        assert n_host > 20
        ref.append((exp, T_host, out_host, n_host))
    # the chain; nothing is fetched and nothing waits until the end
    b = device_buffers(ctx)
    d_T = upload(np.stack([T4, T4b]))[0]
    cands = [_Cand(rec, cp, outl, cap, T=d_T[c]) for c, (rec, (cp, outl)) in enumerate(zip(recs, held))]
    rows = _Rows(cap, 2, has_fill=0)  # the pose problems span the capacity: no point beyond the frame's keypoints
    d_recs = upload_records([c.record(api) for c in cands])
    d_keys = ctx.device_keys_un(0, st.cuda_stream)
    st.synchronize()
    keys2 = raw(d_keys, 28 * cap).repeat(2)
    ur2 = raw(b["u_right"], 4 * cap).repeat(2)
    d_off = upload(np.array([0, cap, 2 * cap], np.int32))[0]
    d_outlier = torch.zeros(2 * cap, dtype=torch.uint8, device="cuda:0")
    d_ninl = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    rows.batch(ctx, d_recs, 2, max(c.n for c in cands), fr["bounds"], True, 1, st)
    ctx._check(ctx.L.orbfe_enqueue_pose_optimization(ctx.h, 2, d_off.data_ptr(), keys2.data_ptr(), ur2.data_ptr(), rows.has.ptr, rows.Xw.ptr,
                                                     d_T.data_ptr(), d_outlier.data_ptr(), d_ninl.data_ptr(), cap, st.cuda_stream))
    st.synchronize()
    got = rows.fetch(cands)
    T_dev, outl_dev, ninl = d_T.cpu().numpy(), d_outlier.cpu().numpy().reshape(2, cap), d_ninl.cpu().numpy()
    for c, (exp, T_host, out_host, n_host) in enumerate(ref):
        _check_row(got, c, nk, cands[c], exp, "candidate %d" % c, has_fill=0)
        assert int(ninl[c]) == n_host, (c, int(ninl[c]), n_host)
        h = exp["has"] != 0
        assert np.array_equal(outl_dev[c][:nk][h], out_host[h]), c
        assert np.abs(T_dev[c] - T_host).max() <= POSE_ATOL, (c, float(np.abs(T_dev[c] - T_host).max()))
    ctx.close()
