"""Initializer::FindHomography + FindFundamental off the GPU: hand-made known answers for the literal model (tests/initializer_model.py;
those of the Jacobi, the inverse and the product are in tests/test_cvmat_model.py), the model against a float64 restatement with numpy.linalg.svd / inv on the committed scenes (tests/initializer_scenes.py), and the C++ host
form (orbslam2_amd/host/Initializer.h, driven by tests/initializer_mirror/mirror_main.cpp) equal to the model bit for bit -- built plain and
as a stand-alone AddressSanitizer + UBSan program."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import host_forms as H
from tests import initializer_model as M
from tests import initializer_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("orbfe_enqueue_find_homography_fundamental", "orbfe_find_homography_fundamental")
F32 = np.float32
# The largest relative deviation of a winner's score, model against the float64 restatement, measured over the two committed scenes on the
# CPU is 9.35e-6 (scene "general", F; "general" H 5.7e-6, "planar" H 3.6e-7, F 4.1e-6).  The bound is 4 times that: headroom for
# conditioning across seeds, not for the kernels or the C++ form, which equal the model bit for bit.
MEASURED_MAX_REL = 9.35e-6
SCORE_REL_TOL = 4 * MEASURED_MAX_REL
MIN_TOP_TWO_GAP = 1e-3   # a condition on a committed scene: its float64 winner leads by at least this, relatively
MARGIN = 1e-3            # flags are compared where every chi-square lies further than this, relatively, from its threshold
MAX_LEFT_OUT = 0.01      # ... and the (hypothesis, match) entries left out are at most this share of a scene


_bits = H.bits


def test_normalize_is_the_sequential_float_sum():
    p = S.scene("general", 63, 12)
    n = M.normalize_keys(p["keys1"])
    x = p["keys1"]["x"].astype(np.float64)
    assert abs(n[0] - x.mean()) < 1e-3 and abs(n[2] - 1 / np.abs(x - x.mean()).mean()) < 1e-6
    acc = F32(0)
    for v in p["keys1"]["x"]:
        acc = F32(acc + v)
    assert n[0] == F32(acc / F32(len(x)))


# ------------------------------------------------------------------ known answers: whole calls
def _small():
    return S.scene("general", 63, 12)


def nan_problem(which):
    """A hypothesis (number 3) whose eight matches share one point.  'shared': the first such match of the small scene for which the
    rank-2 system's homography is so close to singular that the transfer error evaluates to NaN.  'at the mean': Normalize's mean of frame 1 is handed over
    as that very point, so six columns of A are zero: H is singular and F21 x1 = (0, 0, c), 0 / 0."""
    p = _small()
    if which == "shared":
        probe = S.solve(S.with_sets(p, np.repeat(np.arange(len(p["pairs"]))[:, None], 8, axis=1)), "nan probe")
        m = int(np.nonzero(np.isnan(probe["all_scores"][0]))[0][0])
        return S.with_sets(p, np.concatenate([p["sets"][:3], [[m] * 8], p["sets"][4:]]))
    q = S.with_sets(p, np.concatenate([p["sets"][:3], [[5] * 8], p["sets"][4:]]))
    i1 = q["pairs"][5, 0]
    q["norm1"] = np.array([q["keys1"]["x"][i1], q["keys1"]["y"][i1], q["norm1"][2], q["norm1"][3]], F32)
    q["norms_given"] = True
    return q


@pytest.mark.parametrize("which", ["shared", "at the mean"])
def test_a_hypothesis_whose_eight_matches_share_one_point_scores_nan_and_never_wins(which):
    q = nan_problem(which)
    base = _small() if which == "shared" else S.fresh(_small(), norm1=q["norm1"])
    clean, r = S.solve(base), S.solve(q)
    assert r["status"] == 0 and r["ok"].all()
    assert np.isnan(r["all_scores"][0, 3]) and (which == "shared" or np.isnan(r["all_scores"][1, 3]))
    assert r["all_scores"].view(np.uint32)[0, 3] == M.NAN_BITS
    if which == "at the mean":
        assert np.array_equal(r["mats"][0][1][3], np.zeros(9, F32))             # H12i = inv of an exactly singular H21i: the zero matrix
    others = np.arange(12) != 3
    assert np.array_equal(_bits(r["all_scores"][:, others]), _bits(clean["all_scores"][:, others]))
    assert (r["best"] != 3).all() and (r["best"] >= 0).all() and not np.isnan(r["score"]).any()
    if (clean["best"] != 3).all():
        assert np.array_equal(r["best"], clean["best"]) and np.array_equal(r["inliers"], clean["inliers"])
    # ... even in front: a NaN never becomes the running maximum
    front = S.with_sets(q, q["sets"][[3, 0, 1, 2]])
    rf = S.solve(front)
    assert np.isnan(rf["all_scores"][0, 0]) and (rf["best"] >= 1).all()


def test_a_scene_where_no_hypothesis_scores_above_zero_has_no_winner():
    p = S.unrelated_frames()
    r = S.solve(p)
    assert r["status"] == 0 and (r["all_scores"] == 0).all()
    assert r["best"].tolist() == [-1, -1] and r["score"].tolist() == [0, 0] and r["H21"] is None and r["F21"] is None
    assert not r["inliers"].any() and r["ninliers"].tolist() == [0, 0]
    o = S.Outputs.expected(p, r)
    assert (o.H21 == S.SENT_F32).all() and (o.F21 == S.SENT_F32).all() and not o.inl_h.any()


def test_of_two_identical_sets_the_first_wins():
    p, r = _small(), S.solve(_small())
    for model in range(2):
        w = int(r["best"][model])
        q = S.with_sets(p, np.concatenate([p["sets"][[w, w]], p["sets"]]))
        rq = S.solve(q)
        assert rq["all_scores"][model, 0] == rq["all_scores"][model, 1] == r["score"][model]
        assert rq["best"][model] == 0 and rq["score"][model] == r["score"][model]
        assert np.array_equal(_bits(rq["H21" if model == 0 else "F21"]), _bits(r["H21" if model == 0 else "F21"]))
    assert M.first_strict_maximum(np.array([0, 2, 2, 3, 3, 1], F32)) == (3, F32(3)) and M.first_strict_maximum(np.array([0, np.nan], F32))[0] == -1


def test_identical_frames_make_every_match_an_inlier_of_every_homography():
    p = S.identical_frames()
    r = S.solve(p)
    N = len(p["pairs"])
    full = F32(0)
    for _ in range(2 * N):
        full = F32(full + M.TH_H)                     # chi-squares below half an ulp of th: every term is th itself
    assert r["best"][0] == 0 and r["score"][0] == full and r["ninliers"][0] == N and r["inliers"][0].all()
    assert (r["all_scores"][0] == full).all()
    H = r["H21"].astype(np.float64) / float(r["H21"][8])
    assert np.abs(H - np.eye(3).reshape(-1)).max() < 1e-3     # the matrix's scale and sign are free
    assert r["ninliers"][1] == N                              # and any F of a pure identity motion is satisfied too


# ------------------------------------------------------------------ the committed scenes
@pytest.mark.parametrize("kind", S.KINDS)
def test_committed_scenes_are_what_they_claim(kind):
    p, r = S.solved_scene(kind)
    assert len(p["pairs"]) == 300 and len(p["sets"]) == 200 and len(p["keys1"]) != len(p["keys2"]) and (p["matches12"] < 0).sum() > 30
    assert 0.12 < p["outlier"].mean() < 0.28 and r["status"] == 0
    assert r["ninliers"][1] > 200 and (r["ninliers"][0] > 200) == (kind == "planar")      # only the plane is a homography
    RH = r["score"][0] / (r["score"][0] + r["score"][1])
    assert (RH > 0.40) == (kind == "planar")                                              # the host's decision (:111-117) falls as it should
    assert r["inliers"][1][p["outlier"]].mean() < 0.2 and r["inliers"][1][~p["outlier"]].mean() > 0.85


@pytest.mark.parametrize("kind", S.KINDS)
def test_model_equals_the_float64_restatement(kind):
    p, r = S.solved_scene(kind)
    f = M.find_f64(p["keys1"], p["keys2"], p["pairs"], p["sets"], p["norm1"], p["norm2"], p["sigma"])
    for model, name in enumerate("HF"):
        top = np.sort(f["scores"][model])[::-1]
        gap = (top[0] - top[1]) / top[0]
        dev = abs(float(r["score"][model]) - f["score"][model]) / f["score"][model]
        chi, th = f["chi"][model], f["th"][model]
        near = (np.abs(chi - th) <= MARGIN * th).any(axis=2)
        flags = (chi <= th).all(axis=2)
        wrong = (flags != r["inliers_all"][model]) & ~near
        print(kind, name, "top-two gap", gap, "winner's deviation", dev, "left out", near.mean(), "flags wrong", int(wrong.sum()))
        assert gap >= MIN_TOP_TWO_GAP, (kind, name, gap)
        assert near.mean() <= MAX_LEFT_OUT, (kind, name, near.mean())
        assert r["best"][model] == f["best"][model], (kind, name)
        assert dev <= SCORE_REL_TOL, (kind, name, dev)
        assert not wrong.any(), (kind, name, np.argwhere(wrong)[:5].tolist())


# ------------------------------------------------------------------ faults
def fault_problem(fault, base=None):
    """One faulty index in the small scene; returns (problem, the hypotheses it makes faulty, the faulty match or None)."""
    p = S.fresh(base if base is not None else _small())
    N, n1, n2 = len(p["pairs"]), len(p["keys1"]), len(p["keys2"])
    m = int(p["sets"][2, 4])                 # a match that at least hypothesis 2 uses
    if fault.startswith("pair"):
        col, value = {"pair idx1 == -1": (0, -1), "pair idx1 == n1": (0, n1), "pair idx2 == -1": (1, -1), "pair idx2 == n2": (1, n2)}[fault]
        p["pairs"][m, col] = value
        return p, np.nonzero((p["sets"] == m).any(axis=1))[0], m
    p["sets"][6, 3] = -1 if fault == "set index == -1" else N
    return p, np.array([6]), None


FAULTS = ["pair idx1 == -1", "pair idx1 == n1", "pair idx2 == -1", "pair idx2 == n2", "set index == -1", "set index == N"]


def check_fault(p, faulty, m, clean, r):
    """What every implementation must show for one fault: status, the faulty hypotheses at 0, every other hypothesis unchanged where the
    faulty match had added nothing (a set fault touches no other hypothesis at all)."""
    assert r["status"] == M.ERR_INVALID and not r["ok"][faulty].any() and r["ok"].sum() == len(r["ok"]) - len(faulty)
    assert (r["all_scores"][:, faulty] == 0).all() and not np.isin(r["best"], faulty).any()
    for model in range(2):
        same = r["ok"].copy() if m is None else r["ok"] & ~clean["added"][model][:, m]
        assert same.sum() >= (len(same) - len(faulty) if m is None else 1)
        assert np.array_equal(_bits(r["all_scores"][model][same]), _bits(clean["all_scores"][model][same]))
    if m is not None:
        assert not r["inliers"][:, m].any()


@pytest.mark.parametrize("fault", FAULTS)
def test_a_faulty_index_is_reported_and_skipped(fault):
    clean = S.solve(_small(), "small")
    p, faulty, m = fault_problem(fault)
    check_fault(p, faulty, m, clean, S.solve(p))


# ------------------------------------------------------------------ the C++ host form
def _run(exe, p, tmp_path):
    problem, result = str(tmp_path / "problem.bin"), str(tmp_path / "out.bin")
    S.write_problem_file(p, problem)
    H.run(exe, problem, result)
    return S.read_result_file(p, result)


def mirror_cases():
    cases = [(kind, S.scene(kind)) for kind in S.KINDS]
    cases += [("N %d, %d sets" % (n, it), S.scene("planar" if n % 2 else "general", n, it)) for n, it in ((8, 1), (9, 2), (63, 12), (65, 65))]
    cases += [("nan " + w, nan_problem(w)) for w in ("shared", "at the mean")]
    cases += [("no winner", S.unrelated_frames()), ("identical frames", S.identical_frames())]
    cases += [(f, fault_problem(f)[0]) for f in FAULTS]
    return cases


@pytest.mark.parametrize("build", H.BUILDS)
def test_cpp_host_form_equals_the_model_bit_for_bit(tmp_path, build):
    exe = H.build(tmp_path, "initializer_mirror", build)
    for what, p in mirror_cases():
        res = S.solve(p)
        want = S.Outputs.expected(p, res)
        norm1, norm2, got = _run(exe, p, tmp_path)
        if not p.get("norms_given"):            # NormalizeKeys of the header against the model's
            assert np.array_equal(_bits(norm1), _bits(p["norm1"])), what
        assert np.array_equal(_bits(norm2), _bits(p["norm2"])), what
        for k in S.Outputs.NAMES:
            a, b = _bits(getattr(got, k)), _bits(getattr(want, k))
            assert np.array_equal(a, b), "%s: %s differs at bytes %s" % (what, k, np.nonzero(a != b)[0][:8].tolist())
    # what the call refuses: nothing is written
    p = S.scene("general", 8, 1)
    for change in (dict(pairs=p["pairs"][:7]), dict(sigma=F32(0)), dict(sigma=F32(-1)), dict(sets=np.zeros((0, 8), np.int32))):
        q = S.fresh(p, **change)
        _, _, got = _run(exe, q, tmp_path)
        blank = S.Outputs(q)
        assert got.status[0] == M.ERR_INVALID
        for k in S.Outputs.NAMES[:-1]:
            assert np.array_equal(_bits(getattr(got, k)), _bits(getattr(blank, k))), (change, k)


def test_the_host_header_includes_nothing_but_the_c_abi_header():
    text = open(H.header("Initializer.h")).read()
    assert H.project_includes(H.header("Initializer.h")) == H.ABI_AND_CVMAT
    assert "opencv" not in text.lower().replace("opencv's", "").replace("no opencv", "")


# ------------------------------------------------------------------ exports and refusals
def test_the_library_exports_both_calls_and_refuses_what_the_arguments_alone_show():
    """Without a device there is no context, and a NULL context is refused too -- so the refusals are told apart by the message."""
    from orbslam2_amd import api
    L = api.load()
    for name in NAMES:
        assert name in api.EXPORTS
        getattr(L, name)  # AttributeError: the symbol is not exported
    assert callable(api.Context.enqueue_find_homography_fundamental) and callable(api.Context.find_homography_fundamental)
    assert L.orbfe_abi_version() == 6
    fn = L.orbfe_enqueue_find_homography_fundamental
    order = ["d_keys1", "n1", "d_keys2", "n2", "d_pairs", "N", "d_sets", "iterations", "norm1", "norm2", "sigma", "d_H21", "d_F21", "d_score", "d_best", "d_inl_h",
             "d_inl_f", "d_ninliers", "d_all", "d_status"]
    norm = (C.c_float * 4)(320, 240, 0.01, 0.01)
    good = dict(d_keys1=8, n1=100, d_keys2=8, n2=120, d_pairs=8, N=50, d_sets=8, iterations=20, norm1=norm, norm2=norm, sigma=1.0, d_H21=8, d_F21=8, d_score=8,
                d_best=8, d_inl_h=8, d_inl_f=8, d_ninliers=8, d_all=8, d_status=8)

    def call(**kw):
        a = dict(good, **kw)
        return fn(None, *[(a[k] or None) if k.startswith("d_") else a[k] for k in order], None), L.orbfe_last_error(None).decode()

    refusals = [(dict(**{k: 0}), "null input") for k in ("d_keys1", "d_keys2", "d_pairs", "d_sets")] + [(dict(norm1=None), "null input"), (dict(norm2=None), "null input")]
    refusals += [(dict(**{k: 0}), "null output") for k in ("d_H21", "d_F21", "d_score", "d_best", "d_status")]
    refusals += [(dict(N=7), "N = 7 < 8"), (dict(N=0), "< 8"), (dict(iterations=0), "iterations = 0 < 1"), (dict(n1=-1), "negative count"),
                 (dict(N=65536), "above its limit"), (dict(iterations=65536), "above its limit"), (dict(n2=(1 << 24) + 1), "above its limit"),
                 (dict(sigma=0.0), "sigma must be > 0"), (dict(sigma=-1.0), "sigma must be > 0"), (dict(sigma=float("nan")), "sigma must be > 0")]
    for kw, message in refusals:
        rc, err = call(**kw)
        assert rc == api.ERR_INVALID and message in err, (kw, rc, err)
    for kw in (dict(), dict(d_inl_h=0, d_inl_f=0, d_ninliers=0, d_all=0), dict(N=8, iterations=1), dict(N=65535, iterations=65535)):
        assert call(**kw) == (api.ERR_INVALID, "null context"), kw
    header = open(os.path.join(ROOT, "include", "orbfe.h")).read()
    assert all("int %s(" % n in header for n in NAMES)
