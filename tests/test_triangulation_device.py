"""ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:652-819) on two device-resident keyframes:
orbfe_enqueue_search_for_triangulation (orbslam2_amd/csrc/orbfe_bow_device.hip).  Every comparison is exact, against the CPU
oracle (orc_search_for_triangulation) and, on the GPU, against the synchronous orbfe_search_for_triangulation as well.  Scenes,
oracle binding and census are in tests/triangulation_scenes.py.

Device arrays are torch tensors, every input over-allocated by PAD zero entries (a check the kernel misses then reads inside the
test's own allocation and shows as a wrong status), every output surrounded by GUARD sentinel cells; the stream is never the
default one.
"""
import ctypes as C

import numpy as np
import pytest

from orbslam2_amd import bow as B
from tests import triangulation_scenes as S
from tests.device_arrays import UNTOUCHED, Guarded, upload

NAME = "orbfe_enqueue_search_for_triangulation"
PAD = 64
FLOORS = dict(pos64=20, pos128=20, pos4096=4, ties=10, flag_changed=10, line_changed=10, disc_changed=4, dist50=3, pruned=10)


# ------------------------------------------------------------------ CPU
def test_the_library_exports_the_call_and_the_keyframe_record():
    from orbslam2_amd import api
    L = api.load()
    assert NAME in api.EXPORTS
    fn = getattr(L, NAME)  # AttributeError: the symbol is not exported
    args = [0 if t is C.c_int else 0.0 if t is C.c_float else None for t in fn.argtypes]
    assert fn(*args) == api.ERR_INVALID
    assert callable(api.Context.enqueue_search_for_triangulation)
    assert C.sizeof(api.TriKeyframe) == 64


def test_the_big_node_scene_exercises_every_class_and_the_census_equals_the_oracle():
    """What keeps the GPU tests from passing on inputs that exercise nothing: in mode (0, 1) the oracle's run over the big-node scene
    has winners beyond the register chunks (64, 128) and beyond the 64 flag bits (4096), ties won by the last candidate, winners
    changed by a flag, by the epipolar-line gate and by the epipole disc, winners at exactly TH_LOW and histogram losers."""
    sc = S.big_node()
    assert (len(sc["kf1"]["k"]), len(sc["kf2"]["k"])) == (306, 4487)
    assert np.hypot(*(sc["epipole"] - np.array([382.0, 228.0]))) < 2
    for mode in S.MODES:
        ref, nref = S.oracle(sc, *mode)
        got, ngot, cls = S.census(sc, *mode)
        print(mode, nref, cls)
        assert ngot == nref and np.array_equal(got, ref), mode
        if mode == (0, 1):
            for k, floor in FLOORS.items():
                assert cls[k] >= floor, (k, cls[k], floor)


def test_the_census_equals_the_oracle_on_the_two_view_scene():
    sc = S.two_view()
    total = 0
    for mode in S.MODES:
        ref, nref = S.oracle(sc, *mode)
        got, ngot, _ = S.census(sc, *mode)
        assert ngot == nref and np.array_equal(got, ref), mode
        total += nref
    assert total > 300


# ------------------------------------------------------------------ helpers (GPU)
def _ctx(api):
    ctx = api.Context(width=640, height=480, nfeatures=1000, fx=S.FX, fy=S.FY, cx=S.CX, cy=S.CY, bf=40.0)
    t = ctx.tables()
    sf, s2 = S.levels()
    assert np.array_equal(t["scale"], sf) and np.array_equal(t["sigma2"], s2)
    return ctx


class _Kf:
    """A keyframe's arrays in HBM and its record.  Edits (name -> array) replace arrays before the upload."""

    def __init__(self, api, kf, nnodes=None, n=None, **edits):
        a = dict(nodes=kf["fv"][0], off=kf["fv"][1], feat=kf["fv"][2], keys=kf["k"], ur=kf["ur"], mp=kf["mp"], desc=kf["d"].reshape(-1))
        a.update(edits)
        self.t = {k: upload(v, pad=PAD) for k, v in a.items()}
        self.n = len(kf["k"]) if n is None else n
        self.nnodes = len(kf["fv"][0]) if nnodes is None else nnodes
        p = [self.t[k][1] for k in ("nodes", "off", "feat", "keys", "ur", "mp", "desc")]
        self.rec = api.TriKeyframe(*p, self.nnodes, self.n)


class _Out:
    """Outputs between guards: match12[n1], pairs[2 * min(n1, n2)], count, status."""

    def __init__(self, n1, n2):
        self.n1, self.np = n1, 2 * min(n1, n2)
        self.g = [Guarded.cells(s) for s in (n1, self.np, 1, 1)]

    def ptr(self, k):
        return self.g[k].ptr

    def fetch(self):
        """(match12, pairs, count, status); asserts that every cell outside them still holds the sentinel."""
        res = [g.fetch() for g in self.g]
        return res[0], res[1], int(res[2][0]), int(res[3][0])


def _enqueue(ctx, sc, k1, k2, mode, out, st, pairs=True):
    ctx.enqueue_search_for_triangulation(k1.rec, k2.rec, sc["F12"], sc["Cw1"], sc["T2w"], S.FX, S.FY, S.CX, S.CY, mode[0], mode[1],
                                         out.ptr(0), out.ptr(2), out.ptr(3), d_pairs=out.ptr(1) if pairs else 0, stream=st.cuda_stream)


def _check(out, ref, nref, pairs=True, what=""):
    m, p, nm, status = out.fetch()
    assert status == 0, (what, status)
    assert nm == nref, (what, nm, nref)
    assert np.array_equal(m, ref), (what, int((m != ref).sum()))
    if pairs:
        assert np.array_equal(p[:2 * nm], S.pairs_of(ref)), what
        assert (p[2 * nm:] == UNTOUCHED).all(), what
    else:
        assert (p == UNTOUCHED).all(), what


def _sync(ctx, sc, mode, mp1=None):
    a, b = sc["kf1"], sc["kf2"]
    return B.search_for_triangulation(ctx, a["fv"], a["k"], a["ur"], a["mp"] if mp1 is None else mp1, a["d"], b["fv"], b["k"], b["ur"], b["mp"], b["d"],
                                      sc["F12"], sc["Cw1"], sc["T2w"], S.FX, S.FY, S.CX, S.CY, mode[0], mode[1])


def _run_scene(api, sc, modes=S.MODES):
    import torch
    ctx = _ctx(api)
    st = torch.cuda.Stream()
    k1, k2 = _Kf(api, sc["kf1"]), _Kf(api, sc["kf2"])
    torch.cuda.synchronize()
    for mode in modes:
        ref, nref = S.oracle(sc, *mode)
        sref, snref = _sync(ctx, sc, mode)
        assert snref == nref and np.array_equal(sref, ref), mode
        for pairs in (True, False):
            out = _Out(k1.n, k2.n)
            _enqueue(ctx, sc, k1, k2, mode, out, st, pairs)
            st.synchronize()
            _check(out, ref, nref, pairs, (mode, pairs))
    ctx.close()


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_gpu_two_view_scene_equals_the_oracle_and_the_synchronous_call():
    from orbslam2_amd import api
    _run_scene(api, S.two_view())


@pytest.mark.gpu
def test_gpu_big_node_scene_equals_the_oracle_and_the_synchronous_call():
    """Nodes of 70, 150 and 4200 KF2 features: list positions beyond the register chunks and beyond the flag register (the CPU test
    above holds the floors of every class).  The three modes run back to back on one context: flags in scratch that survived a
    call would change the next."""
    from orbslam2_amd import api
    _run_scene(api, S.big_node())


@pytest.mark.gpu
def test_gpu_flags_another_matcher_left_in_the_shared_scratch_do_not_reach_the_search():
    """The flags of list positions from 4096 on are bytes of the context's BoW scratch, indexed by idx2, which
    orbfe_enqueue_search_by_bow_kf uses too and which no launch sweeps: the lane that owns such a position zeroes its byte before the
    node's first query.  On one context and one stream: the bow_kf big-node call (a KF2 node of 4200 keypoints), whose winners past
    position 4096 leave set bytes; directly behind it the big-node search in mode (0, 1), some of whose winners lie on those bytes;
    then the same search again, behind its own set bytes."""
    import torch
    from orbslam2_amd import api
    from tests import bow_kf_scenes as K

    def late(fv):
        return np.concatenate([fv[2][fv[1][i]:fv[1][i + 1]][4096:] for i in range(len(fv[0]))])

    b1, b2 = K.big_node()
    sc = S.big_node()
    bref, bnref = K.oracle(b1, b2, 0.75, True)
    ref, nref = S.oracle(sc, 0, 1)
    stale = np.intersect1d(bref[bref >= 0], late(b2["fv"]))
    assert np.intersect1d(stale, np.intersect1d(ref[ref >= 0], late(sc["kf2"]["fv"]))).size > 0  # a byte left set would cost a winner
    ctx = _ctx(api)
    st = torch.cuda.Stream()
    held, recs = [], []
    for kf in (b1, b2):
        t = [upload(v, pad=PAD) for v in (kf["fv"][0], kf["fv"][1], kf["fv"][2], kf["valid"], kf["d"].reshape(-1), kf["ang"])]
        held.append(t)
        recs.append(api.BowKeyframe(*[p for _, p in t], None, len(kf["fv"][0]), len(kf["d"])))
    k1, k2 = _Kf(api, sc["kf1"]), _Kf(api, sc["kf2"])
    bout = [Guarded.cells(s) for s in (len(b1["d"]), 1, 1)]
    first, second = _Out(k1.n, k2.n), _Out(k1.n, k2.n)
    torch.cuda.synchronize()
    ctx.enqueue_search_by_bow_kf(recs[0], recs[1], 0.75, True, bout[0].ptr, bout[1].ptr, bout[2].ptr, d_pairs=0, stream=st.cuda_stream)
    _enqueue(ctx, sc, k1, k2, (0, 1), first, st)
    _enqueue(ctx, sc, k1, k2, (0, 1), second, st)
    st.synchronize()
    bm, bnm, bstatus = (g.fetch() for g in bout)
    assert bstatus[0] == 0 and bnm[0] == bnref and np.array_equal(bm, bref)
    _check(first, ref, nref, True, "behind bow_kf")
    _check(second, ref, nref, True, "behind itself")
    ctx.close()


@pytest.mark.gpu
def test_gpu_node_size_edges_every_step_a_tie_that_takes_a_flag():
    import torch
    from orbslam2_amd import api
    ctx = _ctx(api)
    st = torch.cuda.Stream()
    for n2 in (1, 63, 64, 65, 128, 129):
        sc = S.single_node(5, n2)
        ref, nref = S.oracle(sc, 0, 1)
        assert nref == min(5, n2) and ref[0] == n2 - 1  # the last of the equals, then the one before it, ...
        k1, k2 = _Kf(api, sc["kf1"]), _Kf(api, sc["kf2"])
        out = _Out(5, n2)
        torch.cuda.synchronize()
        _enqueue(ctx, sc, k1, k2, (0, 1), out, st)
        st.synchronize()
        _check(out, ref, nref, True, n2)
    ctx.close()


@pytest.mark.gpu
def test_gpu_create_new_map_points_loop_patches_has_mp_on_the_stream():
    """KF1 against three neighbours queued on one stream without a host synchronise in between; after each call a torch op on the
    same stream gives every other matched KF1 keypoint a map point, as CreateNewMapPoints does between two neighbours."""
    import torch
    from orbslam2_amd import api
    ctx = _ctx(api)
    st = torch.cuda.Stream()
    base = S.two_view()
    scs = [dict(base, kf2=S.view_of(seed)) for seed in (2, 3, 4)]
    n1 = len(base["kf1"]["k"])
    k1 = _Kf(api, base["kf1"])
    k2s = [_Kf(api, sc["kf2"]) for sc in scs]
    outs = [_Out(n1, n1) for _ in scs]
    has_mp = k1.t["mp"][0]
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        for sc, k2, out in zip(scs, k2s, outs):
            _enqueue(ctx, sc, k1, k2, (0, 1), out, st)
            m = out.g[0].view[:n1]
            hit = (m >= 0).to(torch.int32)
            every_other = (hit.cumsum(0) % 2 == 1) & (m >= 0)  # the 1st, 3rd, ... matched idx1
            has_mp[:n1] |= every_other.to(torch.uint8)
    st.synchronize()
    mp1 = base["kf1"]["mp"].copy()
    total = 0
    for sc, out in zip(scs, outs):
        ref, nref = S.oracle(sc, 0, 1, mp1=mp1)
        _check(out, ref, nref, True, "neighbour")
        i1 = np.nonzero(ref >= 0)[0]
        mp1[i1[::2]] = 1
        total += nref
    assert total > 300 and np.array_equal(has_mp[:n1].cpu().numpy(), mp1)
    ctx.close()


@pytest.mark.gpu
def test_gpu_empty_shapes_give_ok_zero_and_all_minus_one():
    import torch
    from orbslam2_amd import api
    ctx = _ctx(api)
    st = torch.cuda.Stream()
    sc = S.big_node()
    a, b = sc["kf1"], sc["kf2"]
    n1, n2 = len(a["k"]), len(b["k"])
    other = (a["fv"][0] + 1000).astype(np.uint32)
    cases = {
        "n1 == 0": (_Kf(api, a, nnodes=0, n=0), _Kf(api, b), (0, 1)),
        "no nodes in KF1": (_Kf(api, a, nnodes=0), _Kf(api, b), (0, 1)),
        "no nodes in KF2": (_Kf(api, a), _Kf(api, b, nnodes=0), (0, 1)),
        "no shared node": (_Kf(api, a, nodes=other), _Kf(api, b), (0, 1)),
        "every KF1 keypoint has a map point": (_Kf(api, a, mp=np.ones(n1, np.uint8)), _Kf(api, b), (0, 1)),
        "every KF2 keypoint has a map point": (_Kf(api, a), _Kf(api, b, mp=np.ones(n2, np.uint8)), (0, 1)),
        "only_stereo without a stereo keypoint": (_Kf(api, a, ur=np.full(n1, -1.0, np.float32)), _Kf(api, b, ur=np.full(n2, -1.0, np.float32)), (1, 1)),
    }
    torch.cuda.synchronize()
    for what, (k1, k2, mode) in cases.items():
        out = _Out(k1.n, k2.n)
        _enqueue(ctx, sc, k1, k2, mode, out, st)
        st.synchronize()
        _check(out, np.full(k1.n, -1, np.int32), 0, True, what)
    ctx.close()


@pytest.mark.gpu
def test_gpu_refused_inputs_are_reported_in_the_status_and_write_nothing_outside_the_outputs():
    import torch
    from orbslam2_amd import api
    ctx = _ctx(api)
    st = torch.cuda.Stream()
    sc = S.big_node()
    a, b = sc["kf1"], sc["kf2"]
    n1, n2 = len(a["k"]), len(b["k"])

    def edit(arr, at, value):
        out = arr.copy()
        out[at] = value
        return out

    # a KF2 keypoint that is a candidate of a usable KF1 keypoint: the oracle's first match
    ref, _ = S.oracle(sc, 0, 0)
    cand2 = int(ref[ref >= 0][0])
    k2_bad_octave = b["k"].copy()
    k2_bad_octave["octave"][cand2] = 8  # nlevels
    cases = {
        "KF1: equal adjacent node ids": (dict(nodes=edit(a["fv"][0], 2, a["fv"][0][1])), {}),
        "KF2: equal adjacent node ids": ({}, dict(nodes=edit(b["fv"][0], 2, b["fv"][0][1]))),
        "KF1: off[k + 1] < off[k]": (dict(off=edit(a["fv"][1], 2, a["fv"][1][1] - 1)), {}),
        "KF2: off[k + 1] < off[k]": ({}, dict(off=edit(b["fv"][1], 2, b["fv"][1][1] - 1))),
        "KF1: off[last] == n + 1": (dict(off=edit(a["fv"][1], -1, n1 + 1)), {}),
        "KF2: off[last] == n + 1": ({}, dict(off=edit(b["fv"][1], -1, n2 + 1))),
        "KF1: a feature index equal to n": (dict(feat=edit(a["fv"][2], 5, n1)), {}),
        "KF2: a feature index equal to n": ({}, dict(feat=edit(b["fv"][2], 5, n2))),
        "KF2: octave == nlevels on a candidate": ({}, dict(keys=k2_bad_octave)),
    }
    assert a["mp"][a["fv"][2][:40]].min() == 0  # node 3, which holds the edited KF2 feature 5, has a usable KF1 keypoint
    torch.cuda.synchronize()
    for what, (e1, e2) in cases.items():
        k1, k2 = _Kf(api, a, **e1), _Kf(api, b, **e2)
        out = _Out(n1, n2)
        _enqueue(ctx, sc, k1, k2, (0, 1), out, st)
        st.synchronize()
        _, _, _, status = out.fetch()  # and the guards
        assert status == api.ERR_INVALID, (what, status)
    # what the host can see is refused by the call itself and queues nothing
    out = _Out(n1, n2)
    k1, k2 = _Kf(api, a), _Kf(api, b)
    for bad1, bad2 in ((api.TriKeyframe(*([None] * 7), 1, n1), k2.rec), (k1.rec, _Kf(api, b, n=65536).rec), (_Kf(api, a, n=-1).rec, k2.rec)):
        with pytest.raises(api.OrbfeError):
            ctx.enqueue_search_for_triangulation(bad1, bad2, sc["F12"], sc["Cw1"], sc["T2w"], S.FX, S.FY, S.CX, S.CY, 0, 1,
                                                 out.ptr(0), out.ptr(2), out.ptr(3), d_pairs=out.ptr(1), stream=st.cuda_stream)
    with pytest.raises(api.OrbfeError):
        ctx.enqueue_search_for_triangulation(k1.rec, k2.rec, sc["F12"], sc["Cw1"], sc["T2w"], S.FX, S.FY, S.CX, S.CY, 0, 1,
                                             0, out.ptr(2), out.ptr(3), stream=st.cuda_stream)
    st.synchronize()
    m, p, _, _ = out.fetch()
    assert (m == UNTOUCHED).all() and (p == UNTOUCHED).all() and out.g[2].untouched() and out.g[3].untouched()
    ctx.close()


@pytest.mark.gpu
def test_gpu_the_synchronous_call_still_equals_the_oracle_on_the_two_view_scene():
    """The epipole and CheckDistEpipolarLine moved into orbfe_epipolar.h, shared with the kernel: the synchronous results may not
    change."""
    from orbslam2_amd import api
    ctx = _ctx(api)
    sc = S.two_view()
    total = 0
    for mode in S.MODES:
        ref, nref = S.oracle(sc, *mode)
        got, ngot = _sync(ctx, sc, mode)
        assert ngot == nref and np.array_equal(got, ref), mode
        total += nref
    assert total > 300
    ctx.close()
