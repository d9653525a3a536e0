"""orbfe_enqueue_find_homography_fundamental and orbfe_find_homography_fundamental (orbslam2_amd/csrc/orbfe_initializer_device.hip):
Initializer::FindHomography + FindFundamental for one frame pair on the device.  Every comparison is exact -- bytes and float bits,
d_all_scores included -- against the literal model (tests/initializer_model.py), which tests/test_initializer_model.py plays against a
float64 restatement and the C++ host form.

Device arrays are torch tensors.  Every input carries FRONT entries before and PAD entries behind its payload (a check the kernel misses
then reads inside the test's own allocation and shows as a wrong score or status); every output lies between GUARD sentinel rows and starts
out as the model's own sentinels, so "untouched" is part of the exact comparison; the stream is never the default one."""
import numpy as np
import pytest

from tests import initializer_model as M
from tests import initializer_scenes as S
from tests.test_initializer_model import FAULTS, fault_problem, nan_problem
from tests.device_arrays import Guarded, upload

FRONT, PAD = 64, 64

OPTIONAL = ("inl_h", "inl_f", "ninliers", "all_scores")


# ------------------------------------------------------------------ helpers
class _Inputs:
    def __init__(self, p):
        self.t = [upload(np.ascontiguousarray(p[k]).reshape(-1), FRONT, PAD) for k in ("keys1", "keys2", "pairs", "sets")]
        self.keys1, self.keys2, self.pairs, self.sets = [t[1] for t in self.t]


class _Block:
    """The outputs of one call in HBM, starting out as the model's sentinels."""

    def __init__(self, p):
        o = S.Outputs(p)
        self.g = {k: Guarded(getattr(o, k)) for k in S.Outputs.NAMES}

    def ptr(self, k):
        return self.g[k].ptr

    def fetch(self):
        return {k: g.fetch() for k, g in self.g.items()}


def _args(p, inp, blk, without=()):
    return dict(d_keys1_un=inp.keys1, n1=len(p["keys1"]), d_keys2_un=inp.keys2, n2=len(p["keys2"]), d_pairs=inp.pairs, n_matches=len(p["pairs"]), d_sets=inp.sets,
                iterations=len(p["sets"]), norm1=p["norm1"], norm2=p["norm2"], sigma=float(p["sigma"]), d_H21=blk.ptr("H21"), d_F21=blk.ptr("F21"),
                d_score=blk.ptr("score"), d_best=blk.ptr("best"), d_status=blk.ptr("status"),
                **{"d_" + {"inl_h": "inliers_h", "inl_f": "inliers_f"}.get(k, k): (0 if k in without else blk.ptr(k)) for k in OPTIONAL})


def _run(ctx, st, p, without=()):
    """Uploads a problem, queues the call, synchronises; returns the outputs as the device left them."""
    import torch
    inp, blk = _Inputs(p), _Block(p)
    torch.cuda.synchronize()  # the uploads above ran on torch's own stream
    ctx.enqueue_find_homography_fundamental(**_args(p, inp, blk, without), stream=st.cuda_stream)
    st.synchronize()
    return blk.fetch()


def _expect(p, res=None, without=()):
    o = S.Outputs.expected(p, res if res is not None else S.solve(p))
    blank = S.Outputs(p)
    return {k: getattr(blank if k in without else o, k) for k in S.Outputs.NAMES}


def _same(got, want, what):
    for k, w in want.items():
        a, b = np.ascontiguousarray(got[k]).view(np.uint8).reshape(-1), np.ascontiguousarray(w).view(np.uint8).reshape(-1)
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, "%s: %s differs in entries %s: %s != %s" % (what, k, (bad // w.dtype.itemsize)[:8].tolist(), got[k].reshape(-1)[(bad // w.dtype.itemsize)[:4]],
                                                                       w.reshape(-1)[(bad // w.dtype.itemsize)[:4]])


@pytest.fixture(scope="module")
def gpu():
    import torch
    from orbslam2_amd import api
    ctx = api.Context(width=S.WIDTH, height=S.HEIGHT, nfeatures=1000, fx=S.FX, fy=S.FY, cx=S.CX, cy=S.CY, bf=40.0)
    yield api, ctx, torch.cuda.Stream()
    ctx.close()


# ------------------------------------------------------------------ exact against the model
SHAPES = [("general", 8, 1), ("planar", 9, 2), ("general", 63, 63), ("planar", 64, 64), ("general", 65, 65), ("planar", 63, 200), ("general", 300, 200),
          ("planar", 300, 200)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n_matches,iterations", SHAPES)
def test_gpu_every_output_equals_the_model_exactly(gpu, kind, n_matches, iterations):
    """Both matrices, both scores, winners, flags, counts and every hypothesis's score of both models, in float bits; n1 != n2."""
    api, ctx, st = gpu
    p, res = S.solved_scene(kind, n_matches, iterations)
    assert len(p["keys1"]) != len(p["keys2"]) and res["status"] == 0 and (n_matches < 63 or (res["best"] >= 0).all())
    want = _expect(p, res)
    for call in range(2):  # the second call: no state is kept between calls, the scratch is reused
        _same(_run(ctx, st, p), want, "%s %d x %d, call %d" % (kind, n_matches, iterations, call))


@pytest.mark.gpu
@pytest.mark.parametrize("without", [OPTIONAL, ("all_scores",), ("inl_h", "ninliers")])
def test_gpu_optional_outputs_may_be_null(gpu, without):
    api, ctx, st = gpu
    p, res = S.solved_scene("general", 63, 63)
    _same(_run(ctx, st, p, without), _expect(p, res, without), "without %s" % (without,))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["nan shared", "nan at the mean", "no winner", "identical frames"])
def test_gpu_degenerate_cases_equal_the_model_exactly(gpu, case):
    """A NaN score (stored as 0x7fc00000) never wins and disturbs no other hypothesis; without a winner the matrices stay untouched,
    best is -1, the score 0 and the flags 0."""
    api, ctx, st = gpu
    p = nan_problem(case[4:]) if case.startswith("nan") else S.unrelated_frames() if case == "no winner" else S.identical_frames()
    res = S.solve(p)
    want = _expect(p, res)
    if case.startswith("nan"):
        assert want["all_scores"].view(np.uint32)[0, 3] == M.NAN_BITS and (want["best"] != 3).all() and (want["best"] >= 0).all()
    elif case == "no winner":
        assert want["best"].tolist() == [-1, -1] and (want["H21"] == S.SENT_F32).all() and (want["F21"] == S.SENT_F32).all() and not want["inl_f"].any()
    else:
        assert want["ninliers"].tolist() == [len(p["pairs"])] * 2
    _same(_run(ctx, st, p), want, case)


@pytest.mark.gpu
@pytest.mark.parametrize("fault", FAULTS)
def test_gpu_what_only_the_device_can_see_is_reported_and_skipped(gpu, fault):
    """One faulty index among good ones: status INVALID, the guards intact, the hypotheses that name it at 0, and every other hypothesis's
    d_all_scores as in the clean call (for a faulty match: wherever that match had added no term).  The faulty values stay inside the
    test's allocations: one entry beyond either end of a padded array."""
    api, ctx, st = gpu
    clean = S.solve(S.scene("general", 63, 12), "small")
    p, faulty, m = fault_problem(fault)
    res = S.solve(p)
    want = _expect(p, res)
    assert want["status"][0] == M.ERR_INVALID
    got = _run(ctx, st, p)
    assert got["status"][0] == api.ERR_INVALID, fault
    _same(got, want, fault)
    assert (got["all_scores"][:, faulty] == 0).all() and not np.isin(got["best"], faulty).any()
    for model in range(2):
        same = res["ok"].copy() if m is None else res["ok"] & ~clean["added"][model][:, m]
        assert same.sum() >= (11 if m is None else 1)
        assert np.array_equal(got["all_scores"][model][same].view(np.uint32), clean["all_scores"][model][same].view(np.uint32)), (fault, model)


@pytest.mark.gpu
def test_gpu_refusals_queue_nothing_and_leave_the_outputs_as_sentinels(gpu):
    import torch
    api, ctx, st = gpu
    p = S.scene("general", 63, 12)
    inp, blk = _Inputs(p), _Block(p)
    good = _args(p, inp, blk)
    refused = [(dict(**{k: 0}), "null input") for k in ("d_keys1_un", "d_keys2_un", "d_pairs", "d_sets")] + [(dict(norm1=None), "null input"), (dict(norm2=None), "null input")]
    refused += [(dict(**{k: 0}), "null output") for k in ("d_H21", "d_F21", "d_score", "d_best", "d_status")]
    refused += [(dict(n_matches=7), "N = 7 < 8"), (dict(iterations=0), "iterations = 0 < 1"), (dict(n1=-1), "negative count"), (dict(n_matches=65536), "above its limit"),
                (dict(iterations=65536), "above its limit"), (dict(n2=(1 << 24) + 1), "above its limit"), (dict(sigma=0.0), "sigma must be > 0"),
                (dict(sigma=-2.0), "sigma must be > 0")]
    torch.cuda.synchronize()
    for kw, message in refused:
        with pytest.raises(api.OrbfeError) as e:
            ctx.enqueue_find_homography_fundamental(**dict(good, **kw), stream=st.cuda_stream)
        assert e.value.code == api.ERR_INVALID and message in str(e.value), kw
    st.synchronize()
    _same(blk.fetch(), _expect(p, without=S.Outputs.NAMES), "after the refusals")
    ctx.enqueue_find_homography_fundamental(**good, stream=st.cuda_stream)      # and the same arguments unchanged are accepted
    st.synchronize()
    _same(blk.fetch(), _expect(p), "accepted")


# ------------------------------------------------------------------ the synchronous form
@pytest.mark.gpu
@pytest.mark.parametrize("kind,n_matches,iterations", [("general", 63, 12), ("planar", 300, 200)])
def test_gpu_the_synchronous_form_on_vmatches12_equals_the_enqueue_form(gpu, kind, n_matches, iterations):
    """vMatches12 with -1 entries is compacted, Normalize runs on the host (the literal header form), the rest is the same call."""
    api, ctx, st = gpu
    p, res = S.solved_scene(kind, n_matches, iterations)
    assert (p["matches12"] < 0).sum() > 10
    dev = _run(ctx, st, p)
    got = ctx.find_homography_fundamental(p["keys1"], p["keys2"], p["matches12"], p["sets"], float(p["sigma"]))
    assert got["n_matches"] == n_matches
    mine = dict(H21=got["H21"].reshape(-1), F21=got["F21"].reshape(-1), score=got["score"], best=got["best"], inl_h=got["inliers_h"], inl_f=got["inliers_f"],
                ninliers=got["ninliers"], all_scores=got["all_scores"])
    _same(mine, {k: dev[k] for k in mine}, "synchronous form against the enqueue form")
    _same(mine, {k: v for k, v in _expect(p, res).items() if k != "status"}, "synchronous form against the model")
    with pytest.raises(api.OrbfeError) as e:   # fewer than eight matches
        few = np.where(np.cumsum(p["matches12"] >= 0) <= 7, p["matches12"], -1)
        ctx.find_homography_fundamental(p["keys1"], p["keys2"], few, p["sets"], 1.0)
    assert e.value.code == api.ERR_INVALID and "N = 7 < 8" in str(e.value)


# ------------------------------------------------------------------ behind SearchForInitialization
@pytest.mark.gpu
def test_gpu_chain_search_for_initialization_then_the_two_models(gpu):
    """Tracking::MonocularInitialization: two small rendered frames are extracted, matched by search_for_initialization, and the matches go
    straight into this call; the model is fed the same matches."""
    from orbslam2_amd import synth
    api, _, st = gpu
    w, h = 480, 320
    left, right = synth.stereo_pair(w, h, seed=7)
    ctx = api.Context(width=w, height=h, nfeatures=600, fx=400.0, fy=400.0, cx=w / 2, cy=h / 2, bf=160.0)
    try:
        out = ctx.stereo_frame(left, right)
        k1, k2 = out["kps_left"], out["kps_right"]
        bounds = (0.0, float(w), 0.0, float(h))
        prev = np.stack([k1["x"], k1["y"]], axis=1)
        matches12, _, n = ctx.search_for_initialization(ctx._view(k1, None, out["desc_left"], bounds), ctx._view(k2, None, out["desc_right"], bounds), prev, 100,
                                                        0.9, True)
        assert n == (matches12 >= 0).sum() and n >= 30
        sets = S.draw_sets(int(n), 40, np.random.default_rng(11))
        p = S.problem(k1, k2, matches12, sets)
        res = S.solve(p)
        assert res["status"] == 0 and (res["best"] >= 0).all() and res["ninliers"].max() >= 8
        got = ctx.find_homography_fundamental(k1, k2, matches12, sets, 1.0)
        mine = dict(H21=got["H21"].reshape(-1), F21=got["F21"].reshape(-1), score=got["score"], best=got["best"], inl_h=got["inliers_h"], inl_f=got["inliers_f"],
                    ninliers=got["ninliers"], all_scores=got["all_scores"])
        _same(mine, {k: v for k, v in _expect(p, res).items() if k != "status"}, "chain, synchronous form")
        _same(_run(ctx, st, p), _expect(p, res), "chain, enqueue form")
    finally:
        ctx.close()
