"""Bag of words on the device-resident frame (orbfe_enqueue_compute_bow, orbfe_enqueue_search_by_bow;
orbslam2_amd/csrc/orbfe_bow_device.hip): Frame::ComputeFboW and ORBmatcher::SearchByFboW(KeyFrame*, Frame&) with device pointers in,
results in HBM, asynchronous on a caller-owned stream.  Every comparison is exact (float weights by their bits), against the CPU
oracle AND against the synchronous entry points (descriptors uploaded, maps and greedy resolve on the host).

Device memory is torch tensors.  Given descriptors and angles become "image slot 0 of the latest extraction call" by one real
extraction call of the same context followed by torch copies into the context's device buffers (_inject, as in
tests/test_matchers_device.py); tests that say "real frame" use what the extraction itself left there.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from orbslam2_amd import bow as B
from tests import test_bow as TB
from tests import test_matchers as TM
from tests.device_arrays import UNTOUCHED, Guarded, context, device_buffers, raw, upload

W, H, FX, FY, CX, CY, BF = TM.W, TM.H, TM.FX, TM.FY, TM.CX, TM.CY, TM.BF
NEW = ["orbfe_enqueue_compute_bow", "orbfe_enqueue_search_by_bow"]
_p = TB._p


# ------------------------------------------------------------------ CPU
def test_the_library_exports_the_bow_enqueue_calls_and_they_refuse_a_null_context():
    from orbslam2_amd import api
    L = api.load()
    for name in NEW:
        assert name in api.EXPORTS
        fn = getattr(L, name)  # AttributeError: the symbol is not exported
        args = [0 if t is C.c_int else 0.0 if t is C.c_float else None for t in fn.argtypes]
        assert fn(*args) == api.ERR_INVALID, name
    for m in ("enqueue_compute_bow", "enqueue_search_by_bow"):
        assert callable(getattr(api.Context, m))


def _no_blocking_variant(kf_fv, kf_valid, kf_d, f_fv, f_d, ratio):
    """SearchByFboW WITHOUT the `frame keypoint already matched` skip of src/ORBmatcher.cc:205-206: every KF feature sees all frame
    features of its node, the last writer keeps a frame keypoint.  What an implementation that ignores the order inside a node
    would compute; the tests assert that the oracle differs from it on their scenes."""
    kb = np.unpackbits(kf_d, axis=1); fb = np.unpackbits(f_d, axis=1)
    out = np.full(len(f_d), -1, np.int32)
    f_at = {int(nid): i for i, nid in enumerate(f_fv[0])}
    for a, nid in enumerate(kf_fv[0]):
        b = f_at.get(int(nid))
        if b is None:
            continue
        ff = f_fv[2][f_fv[1][b]:f_fv[1][b + 1]]
        kk = kf_fv[2][kf_fv[1][a]:kf_fv[1][a + 1]]
        dist = (kb[kk][:, None, :] != fb[ff][None, :, :]).sum(axis=2)
        for r, real_kf in enumerate(kk):
            if not kf_valid[real_kf]:
                continue
            row = dist[r]
            j = int(row.argmin())  # the first minimum
            best1 = int(row[j])
            best2 = int(np.delete(row, j).min()) if len(row) > 1 else 256
            if best1 <= 50 and np.float32(best1) < np.float32(ratio) * np.float32(best2):
                out[ff[j]] = real_kf
    return out


def test_the_in_node_order_matters_on_the_test_scene():
    """CPU: on the scene of the GPU tests the oracle's greedy rule and the `no blocking` variant disagree at every ratio and
    level used, so a device path that lost the order inside a node cannot pass them."""
    sc = _scene()
    L, v = TB._oracle_voc(sc["vocab"])
    for level in (4, 2):
        _, _, kf_fv = TB._oracle_transform(L, v, sc["kf_d"], level)
        _, _, f_fv = TB._oracle_transform(L, v, sc["f_d"], level)
        for ratio in (0.7, 0.75, 0.95):
            ref, nref = _oracle_search(L, kf_fv, sc["kf_valid"], sc["kf_d"], sc["kf_ang"], f_fv, sc["f_d"], sc["f_ang"], ratio, False)
            var = _no_blocking_variant(kf_fv, sc["kf_valid"], sc["kf_d"], f_fv, sc["f_d"], ratio)
            print("level %d ratio %.2f: %d matches, variant differs at %d" % (level, ratio, nref, int((var != ref).sum())))
            assert nref > 300 and (var != ref).any(), (level, ratio)
    L.orc_vocab_destroy(v)


# ------------------------------------------------------------------ helpers
_VOCAB = {}


def _vocab():
    if "small" not in _VOCAB:
        _VOCAB["small"] = B.build_vocabulary(TB._descs(1, 6000), k=10, levels=5, seed=7)  # the vocabulary of tests/test_bow.py
    return _VOCAB["small"]


def _scene():
    """The scene of test_gpu_bow_transform_and_search (tests/test_bow.py), same seeds and draw order."""
    kf_d = TB._descs(4, 1500)
    rng = np.random.default_rng(5)
    perm = rng.permutation(1500)[:1200]
    f_d = np.concatenate([TB._descs(6, 0, base=kf_d[perm], flip=0.04), TB._descs(7, 400)])
    kf_valid = (rng.random(len(kf_d)) < 0.8).astype(np.int32)
    kf_ang = rng.uniform(0, 360, len(kf_d)).astype(np.float32)
    f_ang = np.concatenate([(kf_ang[perm] + rng.normal(0, 5, 1200)) % 360, rng.uniform(0, 360, 400)]).astype(np.float32)
    return dict(vocab=_vocab(), kf_d=kf_d, f_d=f_d, kf_valid=kf_valid, kf_ang=kf_ang, f_ang=f_ang, rng=rng)


def _oracle_search(L, kf_fv, kf_valid, kf_d, kf_ang, f_fv, f_d, f_ang, ratio, ori):
    ref = np.zeros(max(len(f_d), 1), np.int32)
    kf_d = np.ascontiguousarray(kf_d); f_d = np.ascontiguousarray(f_d)
    nref = L.orc_search_by_bow(_p(kf_fv[0]), _p(kf_fv[1]), _p(kf_fv[2]), len(kf_fv[0]), _p(kf_valid), _p(kf_d), _p(kf_ang),
                               _p(f_fv[0]), _p(f_fv[1]), _p(f_fv[2]), len(f_fv[0]), _p(f_d), _p(f_ang), len(f_d), ratio, int(ori), _p(ref))
    return ref[: len(f_d)], nref


def _inject(ctx, k, d, ur, seed=501):
    """Makes (k, d, ur) image slot 0 of a fresh extraction call of `ctx` (see the module docstring)."""
    import torch
    from orbslam2_amd import synth
    left, right = synth.stereo_pair(ctx.width, ctx.height, seed=seed)
    ctx.stereo_frame(left, right)
    n = len(k)
    assert n <= ctx.capacity
    b = device_buffers(ctx)
    raw(b["kps"], 28 * ctx.capacity)[: 28 * n] = upload(np.ascontiguousarray(k, O.KP_DTYPE))[0]
    raw(b["desc"], 32 * ctx.capacity)[: 32 * n] = upload(np.ascontiguousarray(d, np.uint8).reshape(-1))[0]
    raw(b["u_right"], 4 * ctx.capacity)[: 4 * n] = upload(np.ascontiguousarray(ur, np.float32).view(np.uint8))[0]
    raw(b["counts"], 4)[:] = upload(np.array([n], np.int32).view(np.uint8))[0]
    torch.cuda.synchronize()


def _inject_desc(ctx, d, angle):
    """Descriptors and angles only: what the two calls read of a slot."""
    k = np.zeros(len(d), O.KP_DTYPE)
    k["angle"] = angle; k["size"] = 31; k["class_id"] = -1
    _inject(ctx, k, d, np.full(len(d), -1.0, np.float32))


def _np(g, dtype=np.int32):
    return g.fetch().view(dtype)


class _Fv:
    """Device outputs of enqueue_compute_bow between guards; 32-bit cells of any type are int32 cells holding UNTOUCHED."""

    def __init__(self, cap):
        self.cap = cap
        self.word_id, self.weight, self.node_id = Guarded.cells(cap), Guarded.cells(cap), Guarded.cells(cap)
        self.words, self.word_w, self.nodes, self.node_feat = Guarded.cells(cap), Guarded.cells(cap), Guarded.cells(cap), Guarded.cells(cap)
        self.node_off = Guarded.cells(cap + 1)
        self.n_words, self.n_nodes, self.status = Guarded.cells(1), Guarded.cells(1), Guarded.cells(1)

    def enqueue(self, ctx, slot, level, stream, per_feature=True):
        pf = dict(d_word_id=self.word_id.ptr, d_weight=self.weight.ptr, d_node_id=self.node_id.ptr) if per_feature else {}
        ctx.enqueue_compute_bow(slot, level, self.words.ptr, self.word_w.ptr, self.n_words.ptr, self.nodes.ptr,
                                self.node_off.ptr, self.node_feat.ptr, self.n_nodes.ptr, self.status.ptr,
                                stream=stream.cuda_stream, **pf)

    def check(self, per, fbow, fv, what="", per_feature=True):
        """After the stream was synchronised: exactly the reference ((word, weight, node) per feature, (words, weights),
        (nodes, off, feat)), nothing written past the counts."""
        n, nw, nn = len(per[0]), len(fbow[0]), len(fv[0])
        assert int(self.status.fetch()[0]) == 0, what
        assert int(self.n_words.fetch()[0]) == nw and int(self.n_nodes.fetch()[0]) == nn, (what, int(self.n_words.fetch()[0]), nw, int(self.n_nodes.fetch()[0]), nn)
        cells = [(self.words, fbow[0], nw), (self.word_w, fbow[1], nw), (self.nodes, fv[0], nn), (self.node_off, fv[1], nn + 1), (self.node_feat, fv[2], n)]
        if per_feature:
            cells += [(self.word_id, per[0], n), (self.weight, per[1], n), (self.node_id, per[2], n)]
        else:
            cells += [(self.word_id, per[0][:0], 0), (self.weight, per[1][:0], 0), (self.node_id, per[2][:0], 0)]
        for i, (t, ref, m) in enumerate(cells):
            got = _np(t)
            assert np.array_equal(got[:m], np.ascontiguousarray(ref[:m]).view(np.int32)), (what, i)  # floats by their bits
            assert (got[m:] == UNTOUCHED).all(), (what, i)


class _Kf:
    """A keyframe's arrays in HBM."""

    def __init__(self, fv, valid, desc, angle, pos=None):
        self.nnodes, self.n = len(fv[0]), len(desc)
        self.keep = [upload(np.ascontiguousarray(x, t))[0] for x, t in ((fv[0], np.uint32), (fv[1], np.int32), (fv[2], np.int32), (valid, np.int32),
                                                                   (desc, np.uint8), (angle, np.float32))]
        self.pos = None if pos is None else upload(np.ascontiguousarray(pos, np.float32))[0]


class _Match:
    def __init__(self, cap, pose=False):
        self.match, self.nm, self.status = Guarded.cells(cap), Guarded.cells(1), Guarded.cells(1)
        self.has = Guarded(np.zeros(cap, np.uint8)) if pose else None
        self.Xw = Guarded(np.zeros((cap, 3), np.float32)) if pose else None

    def enqueue(self, ctx, slot, kf, fv, ratio, ori, stream, kf_nnodes=None):
        p = [t.data_ptr() if t.numel() else 0 for t in kf.keep]
        ctx.enqueue_search_by_bow(slot, p[0], p[1], p[2], kf.nnodes if kf_nnodes is None else kf_nnodes, p[3], p[4], p[5], kf.n,
                                  fv.nodes.ptr, fv.node_off.ptr, fv.node_feat.ptr, fv.n_nodes.ptr, ratio, ori,
                                  self.match.ptr, self.nm.ptr, self.status.ptr,
                                  d_kf_pos=0 if kf.pos is None else kf.pos.data_ptr(), d_has_point=0 if self.has is None else self.has.ptr,
                                  d_Xw=0 if self.Xw is None else self.Xw.ptr, stream=stream.cuda_stream)

    def check(self, ref, nref, what=""):
        got = _np(self.match)
        n = len(ref)
        assert int(self.status.fetch()[0]) == 0, what
        assert int(self.nm.fetch()[0]) == nref, (what, int(self.nm.fetch()[0]), nref)
        assert np.array_equal(got[:n], ref), (what, int((got[:n] != ref).sum()))
        assert (got[n:] == UNTOUCHED).all(), what


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["small", "full"])
def test_gpu_compute_bow_on_an_injected_frame(which):
    """1. Vocabulary and descriptors of tests/test_bow.py at levels 4, 2, 0 (one node holds everything) and 9 (deeper than the
    tree); the full-size vocabulary at level 4.  == oracle, == the synchronous transform + maps."""
    import torch
    from orbslam2_amd import api
    if which == "small":
        blob, levels = _vocab(), (4, 2, 0, 9)
        d = TB._descs(4, 1500)
    else:
        blob, levels = B.build_full_vocabulary(), (4,)
        rng = np.random.default_rng(3)
        data = np.frombuffer(blob, np.uint8, offset=8 + 120).reshape(-1, 408)
        leaves = data[rng.integers(11111, 111111, 1300), 8:8 + 320].reshape(1300, 10, 32)[np.arange(1300), rng.integers(0, 10, 1300)]
        d = np.concatenate([leaves ^ np.packbits(rng.random((1300, 256)) < 0.02, axis=1, bitorder="little"), rng.integers(0, 256, (200, 32)).astype(np.uint8)])
    ctx = context(api)
    st = torch.cuda.Stream()
    out = _Fv(ctx.capacity)
    _inject_desc(ctx, d, np.zeros(len(d), np.float32))
    with pytest.raises(api.OrbfeError):
        out.enqueue(ctx, 0, 4, st)  # no vocabulary yet: refused on the host
    B.vocab_load(ctx, blob)
    L, v = TB._oracle_voc(blob)
    for level in levels:
        per, fbow, fv = TB._oracle_transform(L, v, d, level)
        if level == 0:
            assert len(fv[0]) == 1
        for per_feature in (True, False):
            out = _Fv(ctx.capacity)
            torch.cuda.synchronize()
            out.enqueue(ctx, 0, level, st, per_feature)
            st.synchronize()
            out.check(per, fbow, fv, (which, level, per_feature), per_feature)
        gw, gwt, gnd = B.transform(ctx, d, level)
        assert np.array_equal(gw, per[0]) and np.array_equal(gwt.view(np.int32), per[1].view(np.int32)) and np.array_equal(gnd, per[2])
        mw, mww, mn, mo, mf = B.maps(gw, gwt, gnd)
        assert np.array_equal(_np(out.words)[: len(mw)].view(np.uint32), mw) and np.array_equal(_np(out.word_w)[: len(mw)], mww.view(np.int32))
        assert np.array_equal(_np(out.nodes)[: len(mn)].view(np.uint32), mn) and np.array_equal(_np(out.node_off)[: len(mo)], mo)
        assert np.array_equal(_np(out.node_feat)[: len(mf)], mf)
    with pytest.raises(api.OrbfeError):
        out.enqueue(ctx, 3, 4, st)  # no such slot
    with pytest.raises(api.OrbfeError):
        out.enqueue(ctx, 0, -1, st)
    L.orc_vocab_destroy(v)
    ctx.close()


@pytest.mark.gpu
def test_gpu_compute_bow_on_real_extracted_frames():
    """2. enqueue_stereo of two pairs, compute_bow on slots 0 and 2 (queued right behind the extraction) == the synchronous transform
    + maps of the fetched descriptors.  The outputs hold a sentinel before: a stale result cannot pass."""
    import torch
    from orbslam2_amd import api, synth
    ctx = context(api, nfeatures=1200, max_images=4)
    B.vocab_load(ctx, _vocab())
    imgs = []
    for seed in (601, 602):
        left, right = synth.stereo_pair(W, H, seed=seed)
        imgs += [left, right]
    d_img = upload(np.stack(imgs).astype(np.uint8))[0]
    st = torch.cuda.Stream()
    outs = {0: _Fv(ctx.capacity), 2: _Fv(ctx.capacity)}
    assert (_np(outs[0].words) == UNTOUCHED).all() and (_np(outs[0].node_feat) == UNTOUCHED).all() and int(outs[0].n_words.fetch()[0]) == UNTOUCHED
    torch.cuda.synchronize()
    ctx.enqueue_stereo(d_img.data_ptr(), 2, st.cuda_stream)
    for slot in (0, 2):
        outs[slot].enqueue(ctx, slot, 4, st)
    st.synchronize()
    seen = []
    for slot in (0, 2):
        d = ctx.fetch_image(slot, stereo=True)["desc"]
        assert len(d) > 300
        gw, gwt, gnd = B.transform(ctx, d, 4)
        mw, mww, mn, mo, mf = B.maps(gw, gwt, gnd)
        outs[slot].check((gw, gwt, gnd), (mw, mww), (mn, mo, mf), slot)
        got = _np(outs[slot].words)[: len(mw)]
        assert (got != UNTOUCHED).all() and int(outs[slot].n_words.fetch()[0]) == len(mw) > 50  # overwritten
        seen.append(got.copy())
    assert not np.array_equal(seen[0], seen[1])  # two different frames
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("level", [4, 2])
def test_gpu_search_by_bow_on_the_injected_scene(level):
    """3. The scene of test_gpu_bow_transform_and_search: == oracle == the synchronous orbfe_search_by_bow at three (ratio, rotation
    check) settings; the frame's feature vector is the one compute_bow left in HBM.  The `no blocking` variant differs from the
    oracle here, so the in-node order is under test; at level 4 the largest shared node is wider than a wave on both sides."""
    import torch
    from orbslam2_amd import api
    sc = _scene()
    L, v = TB._oracle_voc(sc["vocab"])
    _, _, kf_fv = TB._oracle_transform(L, v, sc["kf_d"], level)
    per, fbow, f_fv = TB._oracle_transform(L, v, sc["f_d"], level)
    shared = np.intersect1d(kf_fv[0], f_fv[0])
    if level == 4:
        big_kf = max(np.diff(kf_fv[1])[np.isin(kf_fv[0], shared)]); big_f = max(np.diff(f_fv[1])[np.isin(f_fv[0], shared)])
        assert len(shared) > 200 and big_kf > 64 and big_f > 64, (len(shared), big_kf, big_f)
    ctx = context(api)
    B.vocab_load(ctx, sc["vocab"])
    _inject_desc(ctx, sc["f_d"], sc["f_ang"])
    st = torch.cuda.Stream()
    fv = _Fv(ctx.capacity)
    kf = _Kf(kf_fv, sc["kf_valid"], sc["kf_d"], sc["kf_ang"])
    torch.cuda.synchronize()
    fv.enqueue(ctx, 0, level, st)
    outs = []
    for ratio, ori in ((0.7, True), (0.75, False), (0.95, True)):
        out = _Match(ctx.capacity)
        out.enqueue(ctx, 0, kf, fv, ratio, ori, st)  # queued back to back, one synchronise below
        outs.append(out)
    st.synchronize()
    fv.check(per, fbow, f_fv, level)
    for out, (ratio, ori) in zip(outs, ((0.7, True), (0.75, False), (0.95, True))):
        ref, nref = _oracle_search(L, kf_fv, sc["kf_valid"], sc["kf_d"], sc["kf_ang"], f_fv, sc["f_d"], sc["f_ang"], ratio, ori)
        assert nref > 300
        out.check(ref, nref, (level, ratio, ori))
        got, ngot = B.search_by_bow(ctx, kf_fv, sc["kf_valid"], sc["kf_d"], sc["kf_ang"], f_fv, sc["f_d"], sc["f_ang"], ratio, ori)
        assert ngot == nref and np.array_equal(got, ref)
        plain, _ = _oracle_search(L, kf_fv, sc["kf_valid"], sc["kf_d"], sc["kf_ang"], f_fv, sc["f_d"], sc["f_ang"], ratio, False)
        var = _no_blocking_variant(kf_fv, sc["kf_valid"], sc["kf_d"], f_fv, sc["f_d"], ratio)
        assert (var != plain).any(), (level, ratio)
    L.orc_vocab_destroy(v)
    ctx.close()


@pytest.mark.gpu
def test_gpu_bow_device_edge_cases():
    """4. A frame without keypoints (flat image, real extraction); a keyframe without nodes; no valid KF feature; a feature index
    out of range on either side; level 0 on both sides (one node holds everything: every loop runs past 64 lanes)."""
    import torch
    from orbslam2_amd import api
    sc = _scene()
    L, v = TB._oracle_voc(sc["vocab"])
    ctx = context(api)
    B.vocab_load(ctx, sc["vocab"])
    st = torch.cuda.Stream()
    _, _, kf_fv = TB._oracle_transform(L, v, sc["kf_d"], 4)
    _, _, f_fv = TB._oracle_transform(L, v, sc["f_d"], 4)
    kf = _Kf(kf_fv, sc["kf_valid"], sc["kf_d"], sc["kf_ang"])
    # the empty slot
    flat = np.full((H, W), 128, np.uint8)
    assert len(ctx.stereo_frame(flat, flat)["kps_left"]) == 0
    fv, out = _Fv(ctx.capacity), _Match(ctx.capacity, pose=True)
    torch.cuda.synchronize()
    fv.enqueue(ctx, 0, 4, st)
    out.enqueue(ctx, 0, kf, fv, 0.7, True, st)
    st.synchronize()
    assert int(fv.status.fetch()[0]) == api.ERR_INVALID and int(fv.n_words.fetch()[0]) == 0 and int(fv.n_nodes.fetch()[0]) == 0
    for t in (fv.words, fv.word_w, fv.nodes, fv.node_off, fv.node_feat, fv.word_id, fv.weight, fv.node_id):
        assert (_np(t) == UNTOUCHED).all()
    assert int(out.status.fetch()[0]) == api.ERR_INVALID and int(out.nm.fetch()[0]) == 0 and (_np(out.match) == UNTOUCHED).all()
    assert not out.has.fetch().any()
    # the scene
    _inject_desc(ctx, sc["f_d"], sc["f_ang"])
    n = len(sc["f_d"])
    none = np.full(n, -1, np.int32)
    fv = _Fv(ctx.capacity)
    torch.cuda.synchronize()
    fv.enqueue(ctx, 0, 4, st)
    out = _Match(ctx.capacity)
    out.enqueue(ctx, 0, kf, fv, 0.7, True, st, kf_nnodes=0)
    st.synchronize()
    out.check(none, 0, "kf_nnodes == 0")
    out = _Match(ctx.capacity)
    out.enqueue(ctx, 0, _Kf(kf_fv, np.zeros_like(sc["kf_valid"]), sc["kf_d"], sc["kf_ang"]), fv, 0.7, True, st)
    st.synchronize()
    out.check(none, 0, "no valid KF feature")
    # an index out of range: the call itself returns ORBFE_OK (enqueue raises otherwise), the device reports it
    shared = np.nonzero(np.isin(kf_fv[0], f_fv[0]))[0]
    bad_feat = kf_fv[2].copy()
    bad_feat[kf_fv[1][shared[3]]] = len(sc["kf_d"]) + 5
    out = _Match(ctx.capacity)
    out.enqueue(ctx, 0, _Kf((kf_fv[0], kf_fv[1], bad_feat), sc["kf_valid"], sc["kf_d"], sc["kf_ang"]), fv, 0.7, True, st)
    st.synchronize()
    assert int(out.status.fetch()[0]) == api.ERR_INVALID
    with pytest.raises(api.OrbfeError):  # the synchronous form sees the same entry on the host
        B.search_by_bow(ctx, (kf_fv[0], kf_fv[1], bad_feat), sc["kf_valid"], sc["kf_d"], sc["kf_ang"], f_fv, sc["f_d"], sc["f_ang"], 0.7, True)
    for bad in (ctx.capacity + 3, n, -2):  # beyond the array, beyond the slot's count, negative
        b = int(np.nonzero(np.isin(f_fv[0], kf_fv[0]))[0][2])
        saved = fv.node_feat.view[int(f_fv[1][b])].item()
        fv.node_feat.view[int(f_fv[1][b])] = bad
        out = _Match(ctx.capacity)
        torch.cuda.synchronize()
        out.enqueue(ctx, 0, kf, fv, 0.7, True, st)
        st.synchronize()
        assert int(out.status.fetch()[0]) == api.ERR_INVALID, bad
        fv.node_feat.view[int(f_fv[1][b])] = saved
    out = _Match(ctx.capacity)
    torch.cuda.synchronize()
    out.enqueue(ctx, 0, kf, fv, 0.7, True, st)  # restored: the oracle's answer again
    st.synchronize()
    out.check(*_oracle_search(L, kf_fv, sc["kf_valid"], sc["kf_d"], sc["kf_ang"], f_fv, sc["f_d"], sc["f_ang"], 0.7, True), what="restored")
    # level 0 on both sides
    _, _, kf0 = TB._oracle_transform(L, v, sc["kf_d"], 0)
    per, fbow, f0 = TB._oracle_transform(L, v, sc["f_d"], 0)
    assert len(kf0[0]) == 1 and len(f0[0]) == 1
    fv = _Fv(ctx.capacity)
    torch.cuda.synchronize()
    fv.enqueue(ctx, 0, 0, st)
    kf = _Kf(kf0, sc["kf_valid"], sc["kf_d"], sc["kf_ang"])
    for ratio, ori in ((0.7, True), (0.95, False)):
        out = _Match(ctx.capacity)
        out.enqueue(ctx, 0, kf, fv, ratio, ori, st)
        st.synchronize()
        ref, nref = _oracle_search(L, kf0, sc["kf_valid"], sc["kf_d"], sc["kf_ang"], f0, sc["f_d"], sc["f_ang"], ratio, ori)
        assert nref > 100
        out.check(ref, nref, ("level 0", ratio))
    fv.check(per, fbow, f0, "level 0")
    L.orc_vocab_destroy(v)
    ctx.close()


@pytest.mark.gpu
def test_gpu_bow_device_at_the_capacity_of_a_large_context():
    """5. nfeatures = 15000 at 1241 x 376 (the default plan accepts it), about 14 000 injected descriptors: the key arrays no longer
    fit one LDS tile, the nodes are hundreds of features wide.  At level 0 the single node holds more features than a lane keeps
    flags for in registers (64 x 64), against a 3000-feature keyframe."""
    import torch
    from orbslam2_amd import api
    ctx = api.Context(width=1241, height=376, nfeatures=15000)
    n = min(14000, ctx.capacity)
    assert n > 64 * 64 + 2048
    blob = _vocab()
    B.vocab_load(ctx, blob)
    L, v = TB._oracle_voc(blob)
    rng = np.random.default_rng(77)
    f_d = TB._descs(8, n)
    f_ang = rng.uniform(0, 360, n).astype(np.float32)
    n_kf = 3000
    src = rng.permutation(n)[:n_kf]
    kf_d = TB._descs(9, 0, base=f_d[src], flip=0.03)
    kf_ang = ((f_ang[src] + rng.normal(0, 5, n_kf)) % 360).astype(np.float32)
    kf_valid = (rng.random(n_kf) < 0.8).astype(np.int32)
    _inject_desc(ctx, f_d, f_ang)
    st = torch.cuda.Stream()
    for level in (4, 0):
        per, fbow, f_fv = TB._oracle_transform(L, v, f_d, level)
        _, _, kf_fv = TB._oracle_transform(L, v, kf_d, level)
        fv = _Fv(ctx.capacity)
        out = _Match(ctx.capacity)
        torch.cuda.synchronize()
        fv.enqueue(ctx, 0, level, st)
        out.enqueue(ctx, 0, _Kf(kf_fv, kf_valid, kf_d, kf_ang), fv, 0.8, True, st)
        st.synchronize()
        fv.check(per, fbow, f_fv, level)
        ref, nref = _oracle_search(L, kf_fv, kf_valid, kf_d, kf_ang, f_fv, f_d, f_ang, 0.8, True)
        assert nref > 100, (level, nref)
        out.check(ref, nref, level)
    L.orc_vocab_destroy(v)
    ctx.close()


@pytest.mark.gpu
def test_gpu_extraction_bow_match_pose_on_one_stream():
    """6. TrackReferenceKeyFrame: enqueue_stereo -> enqueue_compute_bow -> enqueue_search_by_bow (has_point / Xw) ->
    orbfe_device_keys_un -> orbfe_enqueue_pose_optimization on one stream with one synchronise.  The keyframe is a perturbed copy
    of the extracted frame (its stereo keypoints back-projected, descriptors with 5 % of the bits flipped).  Matches equal the
    oracle's; pose, outlier flags and inlier count are bit-equal to the host entry point fed the same arrays."""
    import torch
    from orbslam2_amd import api, synth
    ctx = context(api, nfeatures=1500)
    blob = _vocab()
    B.vocab_load(ctx, blob)
    L, v = TB._oracle_voc(blob)
    left, right = synth.stereo_pair(W, H, seed=701)
    d_img = upload(np.stack([left, right]).astype(np.uint8))[0]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    ctx.enqueue_stereo(d_img.data_ptr(), 1, st.cuda_stream)
    ctx.synchronize(st.cuda_stream)
    fr = ctx.fetch_image(0, stereo=True)
    k, d, ur = fr["kps"], fr["desc"], fr["u_right"]
    s = TM._frame_scene(k, d, ur, 701)
    level = 4
    per, fbow, f_fv = TB._oracle_transform(L, v, d, level)
    _, _, kf_fv = TB._oracle_transform(L, v, s["desc"], level)
    ref, nref = _oracle_search(L, kf_fv, s["valid"], s["desc"], s["angle"], f_fv, d, np.ascontiguousarray(k["angle"]), 0.7, True)
    assert nref > 40
    T0 = np.eye(4, dtype=np.float32); T0[:3] = s["T_cur"]
    has_point = (ref >= 0).astype(np.uint8)
    Xw = np.zeros((len(k), 3), np.float32); Xw[ref >= 0] = s["pos"][ref[ref >= 0]]
    T_host, out_host, n_host = ctx.pose_optimization(T0, k, ur, has_point, Xw)
    assert n_host > 20
    # the chain; nothing is fetched and nothing waits until the end
    b = device_buffers(ctx)
    kf = _Kf(kf_fv, s["valid"], s["desc"], s["angle"], s["pos"])
    fv, out = _Fv(ctx.capacity), _Match(ctx.capacity, pose=True)
    d_T = upload(T0)[0]
    d_off = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    d_outlier = torch.zeros(ctx.capacity, dtype=torch.uint8, device="cuda:0")
    d_ninl = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    counts = raw(b["counts"], 4).view(torch.int32)
    torch.cuda.synchronize()
    ctx.enqueue_stereo(d_img.data_ptr(), 1, st.cuda_stream)
    fv.enqueue(ctx, 0, level, st)
    out.enqueue(ctx, 0, kf, fv, 0.7, True, st)
    d_keys = ctx.device_keys_un(0, st.cuda_stream)
    with torch.cuda.stream(st):
        d_off[1:2] = counts  # offsets = [0, the slot's keypoint count], on the device
    ctx._check(ctx.L.orbfe_enqueue_pose_optimization(ctx.h, 1, d_off.data_ptr(), d_keys, b["u_right"], out.has.ptr, out.Xw.ptr,
                                                     d_T.data_ptr(), d_outlier.data_ptr(), d_ninl.data_ptr(), ctx.capacity, st.cuda_stream))
    st.synchronize()
    fv.check(per, fbow, f_fv)
    out.check(ref, nref)
    n = len(k)
    assert np.array_equal(out.has.fetch()[:n], has_point) and np.array_equal(out.Xw.fetch()[:n], Xw)
    assert np.array_equal(d_T.cpu().numpy(), T_host) and int(d_ninl.item()) == n_host
    assert np.array_equal(d_outlier.cpu().numpy()[:n][ref >= 0], out_host[ref >= 0])
    L.orc_vocab_destroy(v)
    ctx.close()
