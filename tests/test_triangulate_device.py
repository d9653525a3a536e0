"""orbfe_enqueue_triangulate_pairs (orbslam2_amd/csrc/orbfe_triangulate_device.hip): the triangulation stage of
LocalMapping::CreateNewMapPoints for pairs that stay in HBM.  Every comparison is exact -- bytes and float bits -- against the literal
model (tests/triangulate_model.py), which tests/test_triangulate_model.py plays against a float64 restatement and the C++ host form.

Device arrays are torch tensors.  Every input carries FRONT entries before and PAD entries behind its payload (a check the kernel misses
then reads inside the test's own allocation and shows as a wrong code or status); every output, both has_mp arrays included, lies between
GUARD sentinel rows and starts out as the model's own sentinels, so "untouched" is part of the exact comparison; the stream is never the
default one."""
import ctypes as C

import numpy as np
import pytest

from tests import triangulate_model as M
from tests import triangulate_scenes as S
from tests.device_arrays import Guarded, upload

FRONT, PAD = 64, 64
UNTOUCHED = S.Outputs.SENT_I32
_cache = {}


# ------------------------------------------------------------------ helpers
class _Kf:
    """A model keyframe in HBM and its record; has_mp is guarded (the call writes it) or a tensor the caller shares with another record."""

    def __init__(self, api, kf, has_mp_ptr=None):
        self.t = {k: upload(v, FRONT, PAD) for k, v in (("keys_un", kf["keys_un"]), ("keys", kf["keys"]), ("ur", kf["ur"]), ("depth", kf["depth"]), ("cos", kf["cos"]))}
        self.mp = None if has_mp_ptr is not None else Guarded(kf["mp"])
        self.kf = kf
        p = [self.t[k][1] for k in ("keys_un", "keys", "ur", "depth", "cos")] + [has_mp_ptr if has_mp_ptr is not None else self.mp.ptr]
        self.rec = api.NewpointKeyframe(*p, (C.c_float * 12)(*kf["Tcw"].tolist()), (C.c_float * 3)(*kf["Ow"].tolist()),
                                        *[float(kf[k]) for k in ("fx", "fy", "cx", "cy", "invfx", "invfy")], kf["n"])


class _Block:
    """The output block of one call in HBM, starting out as the model's sentinels."""

    def __init__(self, p, n_rows, rows_used):
        o = S.Outputs(p, n_rows, rows_used)
        self.code, self.x3d, self.new = Guarded(o.code), Guarded(o.x3d), Guarded(o.new)
        self.nnew, self.status = Guarded(np.array([UNTOUCHED], np.int32)), Guarded(np.array([UNTOUCHED], np.int32))
        self.pos = None if n_rows is None else Guarded(o.pos)
        self.used = Guarded(np.array([rows_used], np.int32))
        self.n_rows = n_rows

    def fetch(self):
        out = dict(code=self.code.fetch(), x3d=self.x3d.fetch(), new=self.new.fetch(), nnew=int(self.nnew.fetch()[0]), status=int(self.status.fetch()[0]),
                   rows_used=int(self.used.fetch()[0]))
        if self.pos is not None:
            out["pos"] = self.pos.fetch()
        return out


def _enqueue(ctx, st, p, k1, k2, d_pairs, d_npairs, blk, patch):
    ctx.enqueue_triangulate_pairs(k1.rec, k2.rec, float(p["mbf"]), float(p["ratio"]), d_pairs, d_npairs, p["max_pairs"], blk.code.ptr, blk.x3d.ptr,
                                  blk.new.ptr, blk.nnew.ptr, blk.status.ptr, d_pos=0 if blk.pos is None else blk.pos.ptr, n_rows=blk.n_rows or 0,
                                  d_rows_used=0 if blk.pos is None else blk.used.ptr, patch_has_mp=patch, stream=st.cuda_stream)


def _run(api, ctx, st, p, n_rows=900, rows_used=11, patch=1):
    """Uploads a problem, queues the call, synchronises; returns the outputs and both has_mp arrays as the device left them."""
    import torch
    k1, k2 = _Kf(api, p["kf1"]), _Kf(api, p["kf2"])
    pairs, npairs = upload(p["pairs"], FRONT, PAD), upload(np.array([p["npairs"]], np.int32), FRONT, PAD)
    blk = _Block(p, n_rows, rows_used)
    torch.cuda.synchronize()  # the uploads above ran on torch's own stream
    _enqueue(ctx, st, p, k1, k2, pairs[1], npairs[1], blk, patch)
    st.synchronize()
    got = blk.fetch()
    got["mp1"], got["mp2"] = k1.mp.fetch(), k2.mp.fetch()
    return got


def _expect(p0, n_rows=900, rows_used=11, patch=1):
    p = S.fresh(p0)
    o = S.Outputs(p, n_rows, rows_used)
    res = S.run_model(p, o, patch)
    want = dict(code=o.code, x3d=o.x3d, new=o.new, nnew=UNTOUCHED if res["nnew"] is None else res["nnew"], status=res["status"],
                rows_used=res["rows_used"], mp1=p["kf1"]["mp"], mp2=p["kf2"]["mp"])
    if n_rows is not None:
        want["pos"] = o.pos
    return want


def _same(got, want, what):
    for k, w in want.items():
        if isinstance(w, np.ndarray):
            a, b = np.ascontiguousarray(got[k]).view(np.uint8).reshape(-1), np.ascontiguousarray(w).view(np.uint8).reshape(-1)
            bad = np.nonzero(a != b)[0]
            item = max(w.nbytes // max(len(w), 1), 1)
            assert bad.size == 0, "%s: %s differs in entries %s" % (what, k, sorted(set((bad // item).tolist()))[:8])
        else:
            assert got[k] == w, (what, k, got[k], w)


def _first(p0, count, extra=3):
    """The first `count` pairs of a problem under a bound of count + extra."""
    return S.problem(p0["kf1"], p0["kf2"], p0["pairs"][:2 * count], max_pairs=count + extra)


@pytest.fixture(scope="module")
def gpu():
    import torch
    from orbslam2_amd import api
    from tests import test_triangulation_device as TT
    ctx = TT._ctx(api)
    sf, s2 = S.levels()
    t = ctx.tables()
    assert np.array_equal(t["scale"], sf) and np.array_equal(t["sigma2"], s2) and ctx.nlevels == S.NLEVELS
    yield api, ctx, torch.cuda.Stream()
    ctx.close()


# ------------------------------------------------------------------ CPU
def _fake_record(api, **fields):
    """A record whose pointers are never followed: the refusals below happen before anything reaches a device."""
    r = api.NewpointKeyframe(8, 8, 8, 8, 8, 8, (C.c_float * 12)(), (C.c_float * 3)(), 1, 1, 1, 1, 1, 1, 10)
    for name, value in fields.items():
        setattr(r, name, value)
    return r


def _refusals(rec_with):
    """(changed arguments, message) for everything the call itself refuses; rec_with(which, **fields) gives a changed record."""
    out = [(dict(kf1=None), "null keyframe record"), (dict(kf2=None), "null keyframe record"), (dict(d_pairs=0), "null d_pairs or d_npairs"),
           (dict(d_npairs=0), "null d_pairs or d_npairs"), (dict(d_code=0), "null output"), (dict(d_x3d=0), "null output"), (dict(d_new=0), "null output"),
           (dict(d_nnew=0), "null output"), (dict(d_status=0), "null output"), (dict(max_pairs=-1), "negative count"), (dict(n_rows=-1), "negative count"),
           (dict(kf1=rec_with(1, n=-1)), "negative count"), (dict(max_pairs=65536), "> 65535"), (dict(d_rows_used=0), "d_pos without d_rows_used")]
    return out + [(dict(kf2=rec_with(2, **{f: None})), "null array in a keyframe record") for f in ("keys_un", "keys", "u_right", "depth", "cos_stereo", "has_mp")]


def test_what_the_arguments_alone_show_is_refused_before_anything_else():
    """Without a device there is no context, and a NULL context is refused too -- so the refusals are told apart by the message."""
    from orbslam2_amd import api
    L = api.load()
    fn = L.orbfe_enqueue_triangulate_pairs
    order = ["kf1", "kf2", "mbf", "ratio_factor", "d_pairs", "d_npairs", "max_pairs", "d_code", "d_x3d", "d_new", "d_nnew", "d_pos", "n_rows", "d_rows_used",
             "patch_has_mp", "d_status"]
    good = dict(kf1=_fake_record(api), kf2=_fake_record(api), mbf=40.0, ratio_factor=1.8, d_pairs=8, d_npairs=8, max_pairs=5, d_code=8, d_x3d=8, d_new=8,
                d_nnew=8, d_pos=8, n_rows=50, d_rows_used=8, patch_has_mp=1, d_status=8)

    def call(**kw):
        a = dict(good, **kw)
        args = [(None if a[k] is None else C.byref(a[k])) if k in ("kf1", "kf2") else (a[k] or None) if k.startswith("d_") else a[k] for k in order]
        return fn(None, *args, None), L.orbfe_last_error(None).decode()

    for kw, message in _refusals(lambda which, **f: _fake_record(api, **f)):
        rc, err = call(**kw)
        assert rc == api.ERR_INVALID and message in err, (kw, rc, err)
    for kw in (dict(), dict(d_pos=0, d_rows_used=0), dict(max_pairs=0, kf2=_fake_record(api, keys=None)), dict(patch_has_mp=0)):
        assert call(**kw) == (api.ERR_INVALID, "null context"), kw


# ------------------------------------------------------------------ GPU: exact against the model
@pytest.mark.gpu
@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 257, 700])
def test_gpu_every_output_equals_the_model_exactly(gpu, count):
    """Codes, float bits of x3D, d_new in pair order, the count, the table rows and the counter, both has_mp arrays; the entries past the
    count, the rows before and behind the appended ones and every guard as they were."""
    api, ctx, st = gpu
    p = _first(S.scene("wide"), count)
    want = _expect(p)
    assert want["status"] == 0 and want["nnew"] == int((want["code"][:count] <= M.CREATED_MAX).sum())
    assert (want["code"][count:] == S.Outputs.SENT_U8).all() and (count < 63 or want["nnew"] > count // 4)
    for call in range(2):  # the second call: no state is kept between calls
        _same(_run(api, ctx, st, p), want, "count %d, call %d" % (count, call))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["narrow", "forward", "degenerate"])
def test_gpu_the_other_scenes_equal_the_model_exactly(gpu, name):
    """Both UnprojectStereo sources, z2 <= 0, reprojection in KF2, w == 0, zero distance, the sweep cap and the selection sort's swaps."""
    api, ctx, st = gpu
    p = S.scene(name)
    want = _expect(p)
    assert want["status"] == 0
    _same(_run(api, ctx, st, p), want, name)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["d_pos == NULL", "patch_has_mp == 0", "keys != keys_un"])
def test_gpu_three_variants_each_alone(gpu, variant):
    api, ctx, st = gpu
    p = S.scene("narrow")
    kw = dict(n_rows=None, rows_used=5) if variant.startswith("d_pos") else dict(patch=0) if variant.startswith("patch") else {}
    if variant.startswith("keys"):
        plain = _expect(p)
        p = S.with_distorted_keys(p)
    want = _expect(p, **kw)
    assert want["status"] == 0 and want["nnew"] > 100
    got = _run(api, ctx, st, p, **kw)
    _same(got, want, variant)
    nnew = want["nnew"]
    if variant.startswith("d_pos"):
        assert (want["new"][:3 * nnew].reshape(-1, 3)[:, 2] == -1).all() and got["rows_used"] == 5 and (want["mp1"] != p["kf1"]["mp"]).any()
    elif variant.startswith("patch"):
        assert np.array_equal(got["mp1"], p["kf1"]["mp"]) and np.array_equal(got["mp2"], p["kf2"]["mp"]) and got["rows_used"] == 11 + nnew
    else:  # only the unprojected points move
        both = (want["code"] <= M.CREATED_MAX) & (plain["code"] <= M.CREATED_MAX)
        moved = (want["x3d"] != plain["x3d"]).any(axis=1) & both
        assert moved.sum() > 20 and set(want["code"][moved].tolist()) <= {M.STEREO1, M.STEREO2}


@pytest.mark.gpu
def test_gpu_a_table_exactly_full_is_accepted_and_one_row_fewer_is_refused_whole(gpu):
    api, ctx, st = gpu
    p = S.scene("narrow")
    nnew = _expect(p)["nnew"]
    full = _expect(p, n_rows=nnew + 5, rows_used=5)
    assert full["status"] == 0 and full["rows_used"] == nnew + 5
    _same(_run(api, ctx, st, p, n_rows=nnew + 5, rows_used=5), full, "exactly full")
    short = _expect(p, n_rows=nnew + 4, rows_used=5)
    assert short["status"] == M.ERR_CAPACITY and short["rows_used"] == 5 and short["nnew"] == nnew
    assert (short["pos"] == np.float32(-555.0)).all() and np.array_equal(short["mp1"], p["kf1"]["mp"]) and np.array_equal(short["mp2"], p["kf2"]["mp"])
    assert np.array_equal(short["code"], full["code"]) and (short["new"][:3 * nnew].reshape(-1, 3)[:, 2] == -1).all()
    got = _run(api, ctx, st, p, n_rows=nnew + 4, rows_used=5)
    assert got["status"] == api.ERR_CAPACITY
    _same(got, short, "one row short")


FAULTS = ["count -1", "count max_pairs + 1", "idx1 == n1", "idx2 == -1", "octave == nlevels", "u_right >= 0 with depth == 0", "*d_rows_used == -1"]


@pytest.mark.gpu
@pytest.mark.parametrize("fault", FAULTS)
def test_gpu_what_only_the_device_can_see_is_reported_and_skipped(gpu, fault):
    """One fault at a time among good pairs: status INVALID, code 11 on that pair only, every other pair equal to the model.  The faulty
    values stay inside the test's allocations: one entry beyond either end of a padded array, a level table of 16 entries for 8 levels."""
    api, ctx, st = gpu
    base = _first(S.scene("narrow"), 131)
    clean = _expect(base)
    p = S.fresh(base)
    pr = p["pairs"].reshape(-1, 2)
    q, kw = int(np.nonzero(clean["code"][60:] <= M.CREATED_MAX)[0][0]) + 60, {}   # a created pair in the middle
    assert clean["status"] == 0 and clean["nnew"] > 20
    if fault == "count -1":
        p["npairs"] = -1
    elif fault == "count max_pairs + 1":
        p["npairs"] = p["max_pairs"] + 1
    elif fault == "idx1 == n1":
        pr[q, 0] = p["kf1"]["n"]
    elif fault == "idx2 == -1":
        pr[q, 1] = -1
    elif fault == "octave == nlevels":
        p["kf1"]["keys_un"]["octave"][pr[q, 0]] = S.NLEVELS
    elif fault.startswith("u_right"):
        p["kf2"]["ur"][pr[q, 1]] = 50.0; p["kf2"]["depth"][pr[q, 1]] = 0.0
    else:
        kw = dict(rows_used=-1)
    want = _expect(p, **kw)
    assert want["status"] == M.ERR_INVALID
    if fault.startswith("count"):
        assert want["nnew"] == UNTOUCHED and (want["code"] == S.Outputs.SENT_U8).all()
    elif fault.startswith("*d_rows_used"):
        assert np.array_equal(want["code"], clean["code"]) and np.array_equal(want["mp1"], base["kf1"]["mp"]) and want["rows_used"] == -1
    else:
        others = np.arange(len(want["code"])) != q
        assert want["code"][q] == M.FAULTY and np.array_equal(want["code"][others], clean["code"][others]) and want["nnew"] == clean["nnew"] - 1
    got = _run(api, ctx, st, p, **kw)
    assert got["status"] == api.ERR_INVALID, fault
    _same(got, want, fault)


@pytest.mark.gpu
def test_gpu_refusals_queue_nothing_and_an_empty_call_writes_status_and_count(gpu):
    import torch
    api, ctx, st = gpu
    p = _first(S.scene("narrow"), 20)
    k1, k2 = _Kf(api, p["kf1"]), _Kf(api, p["kf2"])
    pairs, npairs = upload(p["pairs"], FRONT, PAD), upload(np.array([p["npairs"]], np.int32), FRONT, PAD)
    blk = _Block(p, 50, 0)
    good = dict(kf1=k1.rec, kf2=k2.rec, mbf=float(p["mbf"]), ratio_factor=float(p["ratio"]), d_pairs=pairs[1], d_npairs=npairs[1], max_pairs=p["max_pairs"],
                d_code=blk.code.ptr, d_x3d=blk.x3d.ptr, d_new=blk.new.ptr, d_nnew=blk.nnew.ptr, d_status=blk.status.ptr, d_pos=blk.pos.ptr, n_rows=50,
                d_rows_used=blk.used.ptr, patch_has_mp=1)

    def rec_with(k, **fields):
        r = api.NewpointKeyframe.from_buffer_copy(k.rec)
        for name, value in fields.items():
            setattr(r, name, value)
        return r

    refused = _refusals(lambda which, **f: rec_with(k1 if which == 1 else k2, **f))
    torch.cuda.synchronize()
    for kw, message in refused:
        with pytest.raises(api.OrbfeError) as e:
            ctx.enqueue_triangulate_pairs(**dict(good, **kw), stream=st.cuda_stream)
        assert e.value.code == api.ERR_INVALID and message in str(e.value), kw
    st.synchronize()
    got = blk.fetch()
    assert got["status"] == UNTOUCHED and got["nnew"] == UNTOUCHED and (got["code"] == S.Outputs.SENT_U8).all() and got["rows_used"] == 0
    assert np.array_equal(k1.mp.fetch(), p["kf1"]["mp"])
    # max_pairs == 0: status 0 and count 0, whatever the records hold; d_code, d_x3d, d_new only have to be non-NULL
    ctx.enqueue_triangulate_pairs(**dict(good, max_pairs=0, kf2=rec_with(k2, keys=None)), stream=st.cuda_stream)
    st.synchronize()
    got = blk.fetch()
    assert (got["status"], got["nnew"], got["rows_used"]) == (0, 0, 0) and (got["code"] == S.Outputs.SENT_U8).all()
    # a count of 0 under a bound: the same, and the table counter stays
    blk2 = _Block(p, 50, 9)
    zero = upload(np.array([0], np.int32), FRONT, PAD)
    torch.cuda.synchronize()
    ctx.enqueue_triangulate_pairs(**dict(good, d_npairs=zero[1], d_code=blk2.code.ptr, d_x3d=blk2.x3d.ptr, d_new=blk2.new.ptr, d_nnew=blk2.nnew.ptr,
                                         d_status=blk2.status.ptr, d_pos=blk2.pos.ptr, d_rows_used=blk2.used.ptr), stream=st.cuda_stream)
    st.synchronize()
    got = blk2.fetch()
    assert (got["status"], got["nnew"], got["rows_used"]) == (0, 0, 9) and (got["code"] == S.Outputs.SENT_U8).all()


# ------------------------------------------------------------------ the loop of CreateNewMapPoints
def _host_loop():
    """The loop as the caller runs it today: the oracle's SearchForTriangulation, the model, the patch, per neighbour."""
    if "loop" not in _cache:
        from tests import triangulation_scenes as TS
        base = TS.two_view()
        scs = [dict(base, kf2=TS.view_of(seed)) for seed in (2, 3, 4)]
        b = TS._two_view_base(1400)
        kf1 = S.from_search_keyframe(base["kf1"], b["T1"])
        kf2s = [S.from_search_keyframe(sc["kf2"], b["T2"]) for sc in scs]
        n1 = kf1["n"]
        steps, rows_used, table = [], 17, np.full((600, 3), np.float32(-555.0), np.float32)
        for sc, kf2 in zip(scs, kf2s):
            ref, nref = TS.oracle(sc, 0, 1, mp1=kf1["mp"])
            p = S.problem(kf1, kf2, TS.pairs_of(ref), max_pairs=n1)   # kf1 and kf2 are shared: the model patches them
            p["mbf"] = np.float32(40.0)
            o = S.Outputs(p, 600, rows_used)
            o.pos = table
            res = S.run_model(p, o, 1)
            assert res["status"] == 0
            steps.append(dict(ref=ref, nref=nref, code=o.code, x3d=o.x3d, new=o.new, nnew=res["nnew"]))
            rows_used = res["rows_used"]
        _cache["loop"] = (scs, kf1, kf2s, steps, rows_used, table, base["kf1"]["mp"], [sc["kf2"]["mp"] for sc in scs])
    return _cache["loop"]


def test_the_host_loop_creates_more_than_a_hundred_points_and_later_neighbours_see_the_patch():
    scs, kf1, kf2s, steps, rows_used, table, mp1_before, _ = _host_loop()
    from tests import triangulation_scenes as TS
    assert rows_used - 17 == sum(s["nnew"] for s in steps) > 100 and all(s["nnew"] > 10 for s in steps)
    unpatched, _ = TS.oracle(scs[2], 0, 1, mp1=mp1_before)
    assert not np.array_equal(unpatched, steps[2]["ref"])


@pytest.mark.gpu
def test_gpu_the_queued_loop_equals_the_host_loop(gpu):
    """KF1 against three neighbours: search, triangulate with patch, three times on one stream, no host synchronise in between, each
    neighbour with its own output block, one table and one row counter for all."""
    import torch
    from tests import test_triangulation_device as TT
    api, ctx, st = gpu
    scs, kf1, kf2s, steps, rows_used, table, mp1_before, mp2_before = _host_loop()
    n1 = kf1["n"]
    t1 = TT._Kf(api, dict(scs[0]["kf1"], mp=mp1_before))
    t2s = [TT._Kf(api, dict(sc["kf2"], mp=mp)) for sc, mp in zip(scs, mp2_before)]
    # the triangulation records share keypoints, mvuRight and has_mp with the search records
    def newpoint(t, kf):
        k = _Kf(api, kf, has_mp_ptr=t.t["mp"][1])
        k.rec.keys_un = k.rec.keys = t.t["keys"][1]; k.rec.u_right = t.t["ur"][1]
        return k
    k1, k2s = newpoint(t1, kf1), [newpoint(t, kf) for t, kf in zip(t2s, kf2s)]
    outs = [TT._Out(n1, n1) for _ in scs]
    p = S.problem(kf1, kf2s[0], [], max_pairs=n1)
    p["mbf"] = np.float32(40.0)
    blks = [_Block(p, 600, 17) for _ in scs]
    pos, used = blks[0].pos, blks[0].used
    torch.cuda.synchronize()
    for sc, t2, k2, out, blk in zip(scs, t2s, k2s, outs, blks):
        TT._enqueue(ctx, sc, t1, t2, (0, 1), out, st)
        ctx.enqueue_triangulate_pairs(k1.rec, k2.rec, 40.0, float(p["ratio"]), out.ptr(1), out.ptr(2), n1, blk.code.ptr, blk.x3d.ptr, blk.new.ptr,
                                      blk.nnew.ptr, blk.status.ptr, d_pos=pos.ptr, n_rows=600, d_rows_used=used.ptr, patch_has_mp=1, stream=st.cuda_stream)
    st.synchronize()
    for i, (out, blk, step) in enumerate(zip(outs, blks, steps)):
        TT._check(out, step["ref"], step["nref"], True, "neighbour %d" % i)
        got = blk.fetch()
        assert got["status"] == 0 and got["nnew"] == step["nnew"], i
        _same(got, dict(code=step["code"], x3d=step["x3d"], new=step["new"]), "neighbour %d" % i)
    assert int(used.fetch()[0]) == rows_used and rows_used - 17 > 100
    _same(dict(pos=pos.fetch()), dict(pos=table), "table")
    assert np.array_equal(t1.t["mp"][0][:n1].cpu().numpy(), kf1["mp"]) and (kf1["mp"] != mp1_before).any()
    for t2, kf2, before in zip(t2s, kf2s, mp2_before):
        assert np.array_equal(t2.t["mp"][0][:n1].cpu().numpy(), kf2["mp"]) and (kf2["mp"] != before).any()


# ------------------------------------------------------------------ chain into a reader
@pytest.mark.gpu
def test_gpu_fuse_reads_the_rows_the_call_has_just_appended(gpu):
    """SearchInNeighbors runs right after: orbfe_enqueue_fuse with an index list over the appended rows, queued behind the triangulation
    with no synchronisation in between, returns what it returns for the same rows uploaded from the model."""
    import torch
    from tests import test_fuse_device as TF
    api, ctx, st = gpu
    p = S.scene("wide")
    base_row, n_rows = 11, 400
    want = _expect(p, n_rows=n_rows, rows_used=base_row)
    nnew = want["nnew"]
    rng = np.random.default_rng(4)
    target = p["kf2"]                                         # the points are fused into KF2, which sees them
    kdesc = rng.integers(0, 256, (target["n"], 32)).astype(np.uint8)
    rows = base_row + np.arange(nnew)
    idx2 = want["new"][:3 * nnew].reshape(-1, 3)[:, 1]
    cols = dict(normal=np.zeros((n_rows, 3), np.float32), max_d=np.zeros(n_rows, np.float32), min_d=np.zeros(n_rows, np.float32),
                desc=rng.integers(0, 256, (n_rows, 32)).astype(np.uint8))
    d = want["pos"][rows] - target["Ow"]
    dist = np.linalg.norm(d, axis=1).astype(np.float32)
    cols["normal"][rows] = d / dist[:, None]
    sf = S.levels()[0]
    cols["max_d"][rows] = dist * sf[target["keys_un"]["octave"][idx2]] * np.float32(0.99)    # PredictScale lands on the keypoint's own level
    cols["min_d"][rows] = cols["max_d"][rows] / sf[-1]
    cols["desc"][rows] = kdesc[idx2] ^ np.packbits(rng.random((nnew, 256)) < 0.03, axis=1, bitorder="little")
    kf = TF._Kf(api, ctx, st, target["keys_un"], kdesc, None, (0.0, 640.0, 0.0, 480.0), 1)
    index, valid = upload(rows.astype(np.int32), pad=TF.PAD)[0], upload(np.ones(nnew, np.int32), pad=TF.PAD)[0]

    class Table:
        def __init__(self, pos_ptr):
            self.n = n_rows
            self.t = [upload(cols[k].reshape(-1), pad=TF.PAD)[0] for k in ("normal", "max_d", "min_d", "desc")]
            self.p = [pos_ptr] + [t.data_ptr() for t in self.t]

        def ptrs(self):
            return self.p

    model_pos = upload(want["pos"].reshape(-1), pad=TF.PAD)[0]
    ref = TF._Out(nnew)
    torch.cuda.synchronize()
    TF._enqueue(ctx, False, kf.rec, target["Tcw"], Table(model_pos.data_ptr()), valid, 3.0, ref, st, n_pts=nnew, d_index=index)
    st.synchronize()
    ref_best, ref_count, ref_status = ref.fetch()
    assert ref_status == 0 and ref_count > nnew // 4 and (ref_best[ref_best >= 0] == idx2[ref_best >= 0]).mean() > 0.8   # the rows decide something
    # the chain: triangulate, then fuse, one synchronise
    k1, k2 = _Kf(api, p["kf1"]), _Kf(api, p["kf2"])
    pairs, npairs = upload(p["pairs"], FRONT, PAD), upload(np.array([p["npairs"]], np.int32), FRONT, PAD)
    blk = _Block(p, n_rows, base_row)
    out = TF._Out(nnew)
    chain = Table(blk.pos.ptr)
    torch.cuda.synchronize()
    _enqueue(ctx, st, p, k1, k2, pairs[1], npairs[1], blk, 1)
    TF._enqueue(ctx, False, kf.rec, target["Tcw"], chain, valid, 3.0, out, st, n_pts=nnew, d_index=index)
    st.synchronize()
    got = blk.fetch()
    got["mp1"], got["mp2"] = k1.mp.fetch(), k2.mp.fetch()
    _same(got, want, "chain")
    TF._check(out, ref_best, ref_count, "fuse behind the triangulation")
