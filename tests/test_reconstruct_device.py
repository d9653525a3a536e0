"""orbfe_enqueue_reconstruct_initial and orbfe_reconstruct_initial (orbslam2_amd/csrc/orbfe_reconstruct_device.hip):
Initializer::ReconstructF / ReconstructH with DecomposeE and CheckRT on the outputs of the RANSAC call, on the device.  Every comparison
is exact -- bytes and float bits, all eight hypotheses and d_codes included -- against the literal model (tests/reconstruct_model.py),
which tests/test_reconstruct_model.py plays against a float64 restatement and the C++ host form.

Device arrays are torch tensors.  Every input carries FRONT entries before and PAD entries behind its payload; every output lies between
GUARD sentinel rows and starts out as the model's own sentinels, so "untouched" is part of the exact comparison; the stream is never the
default one."""
import numpy as np
import pytest

from tests import initializer_scenes as S
from tests import reconstruct_model as R
from tests import reconstruct_scenes as RS
from tests.device_arrays import Guarded, upload
from tests.test_reconstruct_model import bad_pair, ngood_problem, truncated

FRONT, PAD = 64, 64
INPUTS = ("keys1", "keys2", "pairs", "H21", "F21", "score", "best", "inl_h", "inl_f")


# ------------------------------------------------------------------ helpers
class _Inputs:
    def __init__(self, q):
        self.t = {k: upload(np.ascontiguousarray(q[k]).reshape(-1), FRONT, PAD) for k in INPUTS}

    def ptr(self, k):
        return self.t[k][1]


class _Block:
    """The outputs of one call in HBM, starting out as the model's sentinels."""

    def __init__(self, q):
        o = RS.Outputs(q)
        self.g = {k: Guarded(getattr(o, k)) for k in RS.Outputs.NAMES}

    def ptr(self, k):
        return self.g[k].ptr

    def fetch(self):
        return {k: g.fetch() for k, g in self.g.items()}


def _args(q, inp, blk, codes=True):
    return dict(d_keys1_un=inp.ptr("keys1"), n1=len(q["keys1"]), d_keys2_un=inp.ptr("keys2"), n2=len(q["keys2"]), d_pairs=inp.ptr("pairs"), n_matches=len(q["pairs"]),
                d_H21=inp.ptr("H21"), d_F21=inp.ptr("F21"), d_score=inp.ptr("score"), d_best=inp.ptr("best"), d_inliers_h=inp.ptr("inl_h"), d_inliers_f=inp.ptr("inl_f"),
                K=q["K"], sigma=float(q["sigma"]), min_triangulated=q["min_triangulated"], model=q["model"], d_model=blk.ptr("model"), d_hyp_R=blk.ptr("hyp_R"),
                d_hyp_t=blk.ptr("hyp_t"), d_ngood=blk.ptr("ngood"), d_cos_parallax=blk.ptr("cos_parallax"), d_result=blk.ptr("result"), d_choice=blk.ptr("choice"),
                d_R21=blk.ptr("R21"), d_t21=blk.ptr("t21"), d_p3d=blk.ptr("p3d"), d_triangulated=blk.ptr("triangulated"), d_codes=blk.ptr("codes") if codes else 0,
                d_status=blk.ptr("status"))


def _run(ctx, st, q, codes=True):
    """Uploads a problem, queues the call, synchronises; returns the outputs as the device left them."""
    import torch
    inp, blk = _Inputs(q), _Block(q)
    torch.cuda.synchronize()  # the uploads above ran on torch's own stream
    ctx.enqueue_reconstruct_initial(**_args(q, inp, blk, codes), stream=st.cuda_stream)
    st.synchronize()
    return blk.fetch()


def _expect(q, res=None, without=()):
    o = RS.Outputs.expected(q, res if res is not None else RS.solve(q))
    blank = RS.Outputs(q)
    return {k: getattr(blank if k in without else o, k) for k in RS.Outputs.NAMES}


def _same(got, want, what):
    for k, w in want.items():
        a, b = np.ascontiguousarray(got[k]).view(np.uint8).reshape(-1), np.ascontiguousarray(w).view(np.uint8).reshape(-1)
        bad = np.nonzero(a != b)[0] // w.dtype.itemsize
        assert bad.size == 0, "%s: %s differs in entries %s: %s != %s" % (what, k, bad[:8].tolist(), np.asarray(got[k]).reshape(-1)[bad[:4]], w.reshape(-1)[bad[:4]])


@pytest.fixture(scope="module")
def gpu():
    import torch
    from orbslam2_amd import api
    ctx = api.Context(width=S.WIDTH, height=S.HEIGHT, nfeatures=1000, fx=S.FX, fy=S.FY, cx=S.CX, cy=S.CY, bf=40.0)
    yield api, ctx, torch.cuda.Stream()
    ctx.close()


# ------------------------------------------------------------------ exact against the model
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 8, 63, 64, 65, 255, 256, 257, 300])
def test_gpu_every_output_equals_the_model_exactly(gpu, n):
    """The first n matches of a 300-match scene, F (chosen by RH on `general`) for odd n and H (chosen by RH on `frontal`) for even n,
    min_triangulated lowered with n so that small problems choose too; n1 != n2."""
    api, ctx, st = gpu
    q = truncated("general" if n % 2 else "frontal", n)
    res = RS.solve(q)
    assert len(q["keys1"]) != len(q["keys2"]) and res["status"] == 0 and res["model"] == n % 2 and res["nhyp"] == (4 if n % 2 else 8)
    assert n < 63 or res["result"] == 0
    want = _expect(q, res)
    for call in range(2):  # the second call: no state is kept between calls, the scratch is reused
        _same(_run(ctx, st, q), want, "%d matches, call %d" % (n, call))


CASES = {
    "general, F by RH, chosen": lambda: RS.scene("general"),
    "frontal, H by RH, chosen": lambda: RS.scene("frontal"),
    "frontal 64, min_triangulated 10": lambda: RS.scene("frontal", 64, 64, 10),
    "planar, H by RH, result 3": lambda: RS.scene("planar"),
    "planar forced to F, result 3": lambda: RS.scene("planar", model=1),
    "general forced to H, result 3": lambda: RS.scene("general", model=0),
    "general forced to F": lambda: RS.scene("general", model=1),
    "no winner, result 1": lambda: RS.fresh(RS.scene("general"), best=np.array([-1, -1], np.int32)),
    "identical frames forced to H, result 2": lambda: RS.identical_frames(0),
    "behind the cameras": lambda: RS.scene("behind", 100, 50),
    "still, code 6": lambda: RS.scene("still", 100, 50),
    "all flags zero, F": lambda: RS.with_flags(RS.scene("general"), 0, 1),
    "all flags zero, H": lambda: RS.with_flags(RS.scene("frontal"), 0, 0),
}
RESULTS = {"general, F by RH, chosen": 0, "frontal, H by RH, chosen": 0, "frontal 64, min_triangulated 10": 0, "planar, H by RH, result 3": 3,
           "planar forced to F, result 3": 3, "general forced to H, result 3": 3, "no winner, result 1": 1, "identical frames forced to H, result 2": 2}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_gpu_models_results_and_degenerate_cases_equal_the_model_exactly(gpu, case):
    api, ctx, st = gpu
    q = CASES[case]()
    res = RS.solve(q)
    if case in RESULTS:
        assert res["result"] == RESULTS[case], (case, res["result"])
    _same(_run(ctx, st, q), _expect(q, res), case)


@pytest.mark.gpu
@pytest.mark.parametrize("ngood", [0, 1, 50, 51, 52])
def test_gpu_the_index_into_the_sorted_cosines(gpu, ngood):
    """min(50, size - 1): the chosen hypothesis counts exactly `ngood` matches."""
    api, ctx, st = gpu
    q, h = ngood_problem(ngood)
    res = RS.solve(q)
    assert res["ngood"][h] == ngood
    _same(_run(ctx, st, q), _expect(q, res), "nGood %d" % ngood)


@pytest.mark.gpu
def test_gpu_codes_may_be_null(gpu):
    api, ctx, st = gpu
    for kind in ("general", "frontal"):
        q, res = RS.solved_scene(kind)
        _same(_run(ctx, st, q, codes=False), _expect(q, res, without=("codes",)), kind + " without d_codes")


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("fault", ["idx1 == -1", "idx1 == n1", "idx2 == -1", "idx2 == n2"])
def test_gpu_a_bad_pair_index_is_reported_and_skipped(gpu, where, fault):
    """Status INVALID, the guards intact, that match code 0 in every hypothesis, every other match as in the clean call.  The faulty
    values stay inside the test's allocations: one entry beyond either end of a padded array."""
    api, ctx, st = gpu
    clean = RS.solve(truncated("general", 65))
    q, m = bad_pair(where, fault)
    res = RS.solve(q)
    want = _expect(q, res)
    assert want["status"][0] == R.ERR_INVALID and not want["codes"][:, m].any()
    got = _run(ctx, st, q)
    assert got["status"][0] == api.ERR_INVALID
    _same(got, want, fault)
    others = np.arange(65) != m
    assert np.array_equal(got["codes"][:, others], clean["codes"][:, others])


@pytest.mark.gpu
def test_gpu_refusals_queue_nothing_and_leave_the_outputs_as_sentinels(gpu):
    import torch
    api, ctx, st = gpu
    q = truncated("general", 65)
    inp, blk = _Inputs(q), _Block(q)
    good = _args(q, inp, blk)
    refused = [(dict(**{k: 0}), "null input") for k in ("d_keys1_un", "d_keys2_un", "d_pairs", "d_H21", "d_F21", "d_score", "d_best", "d_inliers_h", "d_inliers_f")]
    refused += [(dict(K=None), "null input")]
    refused += [(dict(**{k: 0}), "null output") for k in ("d_model", "d_hyp_R", "d_hyp_t", "d_ngood", "d_cos_parallax", "d_result", "d_choice", "d_R21", "d_t21", "d_p3d",
                                                          "d_triangulated", "d_status")]
    refused += [(dict(n_matches=0), "N = 0 < 1"), (dict(n1=-1), "negative count"), (dict(n_matches=65536), "above its limit"), (dict(n2=(1 << 24) + 1), "above its limit"),
                (dict(sigma=0.0), "sigma must be > 0"), (dict(sigma=-2.0), "sigma must be > 0"), (dict(K=[0.0, 520.0, 320.0, 240.0]), "fx and fy must be > 0"),
                (dict(K=[520.0, -1.0, 320.0, 240.0]), "fx and fy must be > 0"), (dict(min_triangulated=-1), "min_triangulated = -1 < 0"),
                (dict(model=2), "outside -1 .. 1"), (dict(model=-2), "outside -1 .. 1")]
    torch.cuda.synchronize()
    for kw, message in refused:
        with pytest.raises(api.OrbfeError) as e:
            ctx.enqueue_reconstruct_initial(**dict(good, **kw), stream=st.cuda_stream)
        assert e.value.code == api.ERR_INVALID and message in str(e.value), kw
    st.synchronize()
    _same(blk.fetch(), _expect(q, without=RS.Outputs.NAMES), "after the refusals")
    ctx.enqueue_reconstruct_initial(**good, stream=st.cuda_stream)      # and the same arguments unchanged are accepted
    st.synchronize()
    _same(blk.fetch(), _expect(q), "accepted")


# ------------------------------------------------------------------ the synchronous form
def _sync(ctx, q, min_parallax, codes=True):
    got = ctx.reconstruct_initial(q["keys1"], q["keys2"], q["pairs"], q["H21"], q["F21"], q["score"], q["best"], q["inl_h"], q["inl_f"], q["K"], float(q["sigma"]),
                                  min_parallax, q["min_triangulated"], q["model"], codes=codes)
    mine = dict(model=np.array([got["model"]], np.int32), ngood=got["ngood"], cos_parallax=got["cos_parallax"], result=np.array([got["result"]], np.int32),
                choice=np.array([got["choice"]], np.int32), p3d=got["p3d"], triangulated=got["triangulated"])
    if codes:
        mine["codes"] = got["codes"]
    return got, mine


@pytest.mark.gpu
def test_gpu_the_synchronous_form_applies_the_parallax_test(gpu):
    """`general`: hypothesis 2 is chosen with a parallax of 5.03 degrees -- accepted under the reference's 1.0, refused under 10.0; the
    other outputs are the enqueue form's either way."""
    api, ctx, st = gpu
    q, res = RS.solved_scene("general")
    want = _expect(q, res)
    deg = np.degrees(np.arccos(float(res["cos_parallax"][res["choice"]])))
    assert res["choice"] == 2 and abs(deg - 5.03) < 0.01
    for min_parallax, ok in ((1.0, True), (10.0, False)):
        got, mine = _sync(ctx, q, min_parallax)
        assert got["ok"] is ok and api.reconstruct_accept(got["model"], got["cos_parallax"][got["choice"]], min_parallax) is ok
        _same(mine, {k: want[k] for k in mine}, "synchronous form, min_parallax %g" % min_parallax)
        n = res["nhyp"]
        _same(dict(R=got["hyp_R"][:n], t=got["hyp_t"][:n], R21=got["R21"].reshape(-1), t21=got["t21"]),
              dict(R=want["hyp_R"][:n], t=want["hyp_t"][:n], R21=want["R21"], t21=want["t21"]), "synchronous form, motions")
        assert not got["hyp_R"][n:].any()       # untouched rows keep the caller's zeros
    got, _ = _sync(ctx, RS.scene("planar"), 1.0, codes=False)       # the H refusal, and codes NULL
    assert got["ok"] is False and got["result"] == 3 and got["codes"] is None and not got["R21"].any()
    bad, _ = bad_pair("last", "idx2 == n2")
    with pytest.raises(api.OrbfeError) as e:
        _sync(ctx, bad, 1.0)
    assert e.value.code == api.ERR_INVALID and "faulty pair index" in str(e.value)


# ------------------------------------------------------------------ behind SearchForInitialization and the RANSAC
@pytest.mark.gpu
def test_gpu_chain_search_ransac_reconstruct_on_one_stream_with_one_synchronise(gpu):
    """Tracking::MonocularInitialization: two small rendered frames are extracted and matched by search_for_initialization; the
    matches go into the RANSAC call, and its outputs are read by this call where they lie: both are queued on one stream and the
    host synchronises once.  The model is run end to end on the same matches."""
    import torch
    from orbslam2_amd import synth
    from tests import test_initializer_device as TI
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
        assert n >= 30
        p = S.problem(k1, k2, matches12, S.draw_sets(int(n), 40, np.random.default_rng(11)))
        ransac = S.solve(p)
        assert ransac["status"] == 0 and (ransac["best"] >= 0).all()
        for model in (-1, 0, 1):
            q = RS.from_ransac(p, ransac, min_triangulated=10, model=model)
            q["K"] = np.array([400.0, 400.0, w / 2, h / 2], np.float32)
            res = RS.solve(q)
            inp, rb = TI._Inputs(p), TI._Block(p)
            unused, blk = _Inputs(q), _Block(q)     # every device input of the second call is the first call's array
            torch.cuda.synchronize()
            ctx.enqueue_find_homography_fundamental(**TI._args(p, inp, rb), stream=st.cuda_stream)
            ctx.enqueue_reconstruct_initial(
                **dict(_args(q, unused, blk), d_keys1_un=inp.keys1, d_keys2_un=inp.keys2, d_pairs=inp.pairs, d_H21=rb.ptr("H21"), d_F21=rb.ptr("F21"),
                       d_score=rb.ptr("score"), d_best=rb.ptr("best"), d_inliers_h=rb.ptr("inl_h"), d_inliers_f=rb.ptr("inl_f")), stream=st.cuda_stream)
            st.synchronize()    # the one synchronise
            TI._same(rb.fetch(), TI._expect(p, ransac), "chain, the RANSAC's outputs")
            _same(blk.fetch(), _expect(q, res), "chain, model %d" % model)
    finally:
        ctx.close()
