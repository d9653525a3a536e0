"""Initializer::ReconstructF / ReconstructH / CheckRT off the GPU: hand-made known answers for the literal model
(tests/reconstruct_model.py), the model against a float64 restatement with numpy.linalg on the scenes of tests/reconstruct_scenes.py, the
census of CheckRT's branches, and the C++ host form (ReconstructInitial of orbslam2_amd/host/Initializer.h, driven by
tests/reconstruct_mirror/mirror_main.cpp) equal to the model bit for bit -- built plain and as a stand-alone AddressSanitizer + UBSan
program."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import host_forms as H
from tests import initializer_scenes as S
from tests import reconstruct_model as R
from tests import reconstruct_scenes as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENSUS = os.path.join(ROOT, "tests", "golden", "reconstruct_census.json")
NAMES = ("orbfe_enqueue_reconstruct_initial", "orbfe_reconstruct_initial")
F32 = np.float32
# Measured here, model against the float64 restatement, over the scenes that choose a hypothesis (general, frontal 300, frontal 64,
# sideways): the largest |R21 - R| element 1.60e-7 (frontal), the largest |t21 - t| element 2.93e-7 (frontal 64), the largest position
# error relative to the point's distance 2.47e-6 (general).  The bounds are 4 times that: headroom for conditioning across seeds, not
# for the kernels or the C++ form, which equal the model bit for bit.
MEASURED_R, MEASURED_T, MEASURED_POS = 1.60e-7, 2.93e-7, 2.47e-6
# Codes are compared where every quantity that the float64 path tests lies further than MARGIN, relatively, from its threshold: the
# errors against th2; a depth against 0 relative to the point's distance.  The cosine's threshold lies 2e-5 below 1 where a float
# cosine resolves 6e-8, so 1e-3 of that distance is below the format's resolution and the margin is 4 float epsilons instead: the
# rounding of dist1 * dist2 and of the quotient.
MARGIN, COS_MARGIN = 1e-3, 4 * float(np.finfo(F32).eps)
MAX_LEFT_OUT = 0.01
# the noise-free sideways scene against the truth, measured: |R21 - I| 2.8e-7, |t21 - (-1, 0, 0)| 5.9e-6 (its only noise is the
# rounding of the pixel coordinates to float); asserted at 4 times that
SIDEWAYS_R, SIDEWAYS_T = 2.8e-7, 5.9e-6

SCENES = {"general": ("general",), "planar": ("planar",), "frontal": ("frontal",), "frontal 64": ("frontal", 64, 64, 10), "sideways": ("sideways", 100, 30),
          "behind": ("behind", 100, 50), "still": ("still", 100, 50), "planar forced F": ("planar", 300, 200, 50, 1), "general forced H": ("general", 300, 200, 50, 0)}
# model, number of inliers, nGood, result, choice: what the issue states for the committed scenes, and what this generator draws for the others
EXPECTED = {"general": (1, 228, [1, 2, 227, 2], 0, 2), "planar": (0, 253, [0, 162, 240, 253, 0, 3, 3, 0], 3, -1), "frontal": (0, 233, [134, 233, 0, 120, 1, 0, 0, 1], 0, 1),
            "frontal 64": (0, 54, [54, 31, 31, 0, 0, 1, 1, 0], 0, 0), "planar forced F": (1, 253, [0, 170, 0, 154], 3, -1),
            "general forced H": (0, 22, [0, 18, 8, 22, 0, 0, 0, 0], 3, -1)}


_bits = H.bits


# ------------------------------------------------------------------ problems shared with the device tests
def truncated(kind, n):
    """The first n matches of the 300-match scene `kind`, min_triangulated lowered with n."""
    q = RS.scene(kind)
    return RS.fresh(q, pairs=q["pairs"][:n].copy(), inl_h=q["inl_h"][:n].copy(), inl_f=q["inl_f"][:n].copy(), min_triangulated=min(50, n // 8))


def ngood_problem(ngood, h=2):
    """`general` forced to F with the flags of exactly `ngood` matches that hypothesis h counts: nGood[h] == ngood."""
    q, res = RS.solved_scene("general", model=1)
    keep = np.nonzero(res["codes"][h] >= 6)[0][:ngood]
    flags = np.zeros_like(q["inl_f"])
    flags[keep] = 1
    return RS.fresh(q, inl_f=flags, min_triangulated=0), h


def bad_pair(where, fault):
    """65 matches of `general` with one pair index outside its frame, at the first or the last match, its inlier flags set."""
    q = truncated("general", 65)
    m = 0 if where == "first" else 64
    col, value = {"idx1 == -1": (0, -1), "idx1 == n1": (0, len(q["keys1"])), "idx2 == -1": (1, -1), "idx2 == n2": (1, len(q["keys2"]))}[fault]
    q["pairs"][m, col] = value
    q["inl_f"][m] = q["inl_h"][m] = 1
    return q, m


def code1_problem():
    """A match triangulated onto the plane at infinity: keypoint 1 at the principal point and keypoint 2 where camera 2 sees the first
    camera's optical axis vanish, so that column 2 of Triangulate's A is exactly zero, the null vector is (0, 0, 1, 0) and its fourth
    component 0.  Returns (problem, hypothesis, match)."""
    q, res = RS.solved_scene("general", model=1)
    q = RS.fresh(q, keys1=q["keys1"].copy(), keys2=q["keys2"].copy())
    m = int(np.nonzero(q["inl_f"])[0][0])
    for h in range(4):
        P2, _ = R.camera2(res["hyp_R"][h].reshape(3, 3), res["hyp_t"][h], q["K"])
        found = []
        for r in range(2):
            up = down = F32(P2[r, 2] / P2[2, 2])
            cands = [up]
            for _ in range(8):          # the quotient and its neighbours: x * P2[2][2] must round to P2[r][2] exactly
                up, down = np.nextafter(up, F32(np.inf)), np.nextafter(down, F32(-np.inf))
                cands += [up, down]
            hit = [c for c in cands if F32(c * P2[2, 2]) == P2[r, 2]]
            if hit:
                found.append(hit[0])
        if len(found) == 2:
            i1, i2 = q["pairs"][m]
            q["keys1"]["x"][i1], q["keys1"]["y"][i1] = q["K"][2], q["K"][3]
            q["keys2"]["x"][i2], q["keys2"]["y"][i2] = found
            return q, h, m
    raise AssertionError("no hypothesis offers exact coordinates")


# ------------------------------------------------------------------ known answers
def test_noise_free_sideways_translation_is_recovered():
    """Exactly one F hypothesis counts every match, and it is the truth: R = I, t = (-1, 0, 0)."""
    q, res = RS.solved_scene(*SCENES["sideways"])
    N = len(q["pairs"])
    assert res["model"] == 1 and res["n_inliers"] == N and (res["ngood"][:4] == N).sum() == 1 and res["result"] == 0
    assert res["ngood"][res["choice"]] == N and res["triangulated"][q["pairs"][:, 0]].all()
    dR, dt = np.abs(res["R21"].reshape(3, 3) - np.eye(3)).max(), np.abs(res["t21"] - np.array([-1.0, 0, 0])).max()
    print("sideways: |R21 - I| %.3g, |t21 - t| %.3g" % (dR, dt))
    assert dR <= 4 * SIDEWAYS_R and dt <= 4 * SIDEWAYS_T
    assert R.accept(1, res["cos_parallax"][res["choice"]], 1.0)


def test_results_1_and_2_are_taken_before_any_hypothesis():
    q = RS.fresh(RS.scene("general"), best=np.array([5, -1], np.int32))       # F is the model by RH and has no winner
    res = RS.solve(q)
    assert (res["model"], res["result"], res["choice"], res["nhyp"]) == (1, 1, -1, 0) and not res["codes"].any() and not res["p3d"].any()
    assert (res["cos_parallax"] == 2.0).all() and not res["ngood"].any()
    res = RS.solve(RS.identical_frames(0))                                      # H = I: d1 / d2 = 1
    assert (res["model"], res["result"], res["choice"], res["nhyp"]) == (0, 2, -1, 0) and not res["codes"].any()
    assert RS.solve(RS.identical_frames(-1))["model"] == 0                      # SH = SF = 2 N th: RH = 0.5


@pytest.mark.parametrize("ngood", [0, 1, 50, 51, 52])
def test_the_index_into_the_sorted_cosines_is_min_50_size_minus_1(ngood):
    q, h = ngood_problem(ngood)
    res = RS.solve(q)
    assert res["ngood"][h] == ngood and res["n_inliers"] == ngood
    if ngood == 0:
        assert res["cos_parallax"][h] == 2.0 and res["choice"] == 0 and not R.accept(1, res["cos_parallax"][0], 0.0) and R.accept(0, res["cos_parallax"][0], 0.0)
        return
    cos = np.sort(res["q"][h]["cos"][res["codes"][h] >= 6])
    assert len(cos) == ngood and res["cos_parallax"][h] == cos[min(50, ngood - 1)]
    assert ngood < 52 or cos[50] != cos[51]     # so that index 50 and index size - 1 are told apart


def test_a_zero_fourth_component_is_a_non_finite_point():
    q, h, m = code1_problem()
    res = RS.solve(q)
    assert res["q"][h]["w"][m] == 0 and res["codes"][h, m] == 1 and res["status"] == 0
    assert not res["triangulated"][q["pairs"][m, 0]] or res["choice"] != h


def test_the_sort_order_of_the_cosines():
    c = np.array([0.5, np.nan, -0.0, 0.0, -1.0, 1.0, -np.nan, 0.99998], F32)
    order = np.argsort(R.order_key(c), kind="stable")
    assert order.tolist() == [4, 2, 3, 0, 7, 5, 1, 6]
    assert R.kth_cosine(c, np.ones(8, bool)).view(np.uint32) == R.NAN_BITS       # index 7 of 8: a NaN, stored with one pattern


def test_the_count_rules():
    assert R.choose_f([227, 227, 0, 0], 228, 50) == -1           # two similar
    assert R.choose_f([0, 150, 227, 158], 228, 50) == 2          # 158 <= 0.7 * 227 = 158.9
    assert R.choose_f([0, 159, 227, 0], 228, 50) == -1
    assert R.choose_f([205, 0, 0, 0], 228, 50) == 0 and R.choose_f([204, 0, 0, 0], 228, 50) == -1      # (int)(0.9 * 228) = 205
    assert R.choose_f([40, 0, 0, 0], 40, 50) == -1 and R.choose_f([40, 0, 0, 0], 40, 40) == 0
    assert R.choose_f([7, 7, 7, 7], 7, 0) == -1 and R.choose_f([0, 0, 0, 0], 0, 0) == 0     # the first of equals, never a later one
    assert R.choose_h([0, 135, 119, 233, 0, 0, 0, 0], 233, 50) == 3 and R.choose_h([0, 175, 119, 233, 0, 0, 0, 0], 233, 50) == -1     # 0.75 * 233 = 174.75
    assert R.choose_h([233, 0, 0, 0, 0, 0, 0, 0], 259, 50) == -1 and R.choose_h([234, 0, 0, 0, 0, 0, 0, 0], 259, 50) == 0       # 0.9 * 259 = 233.1
    assert R.choose_h([50, 0, 0, 0, 0, 0, 0, 0], 50, 50) == -1 and R.choose_h([0] * 8, 0, 0) == -1
    assert R.choose_h([10, 20, 30, 29, 0, 0, 0, 0], 30, 5) == -1  # the second best is found behind the best as well as before it


# ------------------------------------------------------------------ the model against float64
def _f64(q, res):
    m = res["model"]
    return R.reconstruct_f64(q["keys1"], q["keys2"], q["pairs"], q["H21"], q["F21"], q["inl_h"] if m == 0 else q["inl_f"], q["K"], q["sigma"], m, q["min_triangulated"])


def _pairing(res, f):
    n = res["nhyp"]
    cost = np.array([[np.abs(res["hyp_R"][i].reshape(3, 3) - f["R"][j]).max() + np.abs(res["hyp_t"][i] - f["t"][j]).max() for j in range(n)] for i in range(n)])
    j = cost.argmin(axis=1)
    assert sorted(j.tolist()) == list(range(n)), "the pairing of hypotheses is no bijection: %s" % j.tolist()
    assert cost[np.arange(n), j].max() < 1e-2
    return j


def _near(g, th2):
    """Entries whose float64 path tests a quantity within the margin of its threshold."""
    near_cos = np.abs(g["cos"] - 0.99998) <= COS_MARGIN
    low = g["cos"] < 0.99998
    reach = np.isfinite(g["z1"])
    near = reach & (np.abs(g["z1"]) <= MARGIN * g["r1"])
    near |= reach & (g["z1"] <= 0) & near_cos
    reach = reach & ~((g["z1"] <= 0) & low)
    near |= reach & (np.abs(g["z2"]) <= MARGIN * g["r2"])
    near |= reach & (g["z2"] <= 0) & near_cos
    reach = reach & ~((g["z2"] <= 0) & low)
    near |= reach & (np.abs(g["err1"] - th2) <= MARGIN * th2)
    reach = reach & ~(g["err1"] > th2)
    near |= reach & (np.abs(g["err2"] - th2) <= MARGIN * th2)
    reach = reach & ~(g["err2"] > th2)
    return near | (reach & near_cos)


@pytest.mark.parametrize("name", list(SCENES))
def test_the_model_against_float64(name):
    q, res = RS.solved_scene(*SCENES[name])
    if name in EXPECTED:
        model, ninl, ngood, result, choice = EXPECTED[name]
        assert (res["model"], res["n_inliers"], res["ngood"][:len(ngood)].tolist(), res["result"], res["choice"]) == (model, ninl, ngood, result, choice)
    f = _f64(q, res)
    assert res["status"] == 0 and f["result"] == res["result"]
    j = _pairing(res, f)
    assert (f["choice"] < 0) == (res["choice"] < 0) and (res["choice"] < 0 or j[res["choice"]] == f["choice"])
    left_out = total = 0
    for h in range(res["nhyp"]):
        fc, mc = f["codes"][j[h]], res["codes"][h]
        near = _near(f["q"][j[h]], f["th2"]) & (fc != 0)
        assert np.array_equal(fc[~near], mc[~near]), (name, h, np.nonzero((fc != mc) & ~near)[0][:8])
        left_out += int(near.sum()); total += len(fc)
    print("%s: %d of %d entries left out" % (name, left_out, total))
    assert left_out <= MAX_LEFT_OUT * total
    if res["choice"] >= 0:
        h = res["choice"]
        counted = res["codes"][h] >= 6
        dR, dt = np.abs(res["R21"].reshape(3, 3) - f["R"][j[h]]).max(), np.abs(res["t21"] - f["t"][j[h]]).max()
        fp = f["p"][j[h]][counted]
        rel = (np.abs(res["p3d"][q["pairs"][counted, 0]] - fp).max(axis=1) / np.linalg.norm(fp, axis=1)).max()
        print("%s: |R21 - R| %.3g, |t21 - t| %.3g, position %.3g relative" % (name, dR, dt, rel))
        assert dR <= 4 * MEASURED_R and dt <= 4 * MEASURED_T and rel <= 4 * MEASURED_POS
        parallax = np.degrees(np.arccos(f["q"][j[h]]["cos"][counted]))
        assert R.accept(res["model"], res["cos_parallax"][h], 1.0) == (np.sort(parallax)[::-1][min(50, len(parallax) - 1)] > 1.0)


def test_the_stated_parallax_of_the_committed_scenes():
    for name, degrees in (("general", 5.03), ("frontal", 28.0)):
        q, res = RS.solved_scene(*SCENES[name])
        assert abs(np.degrees(np.arccos(float(res["cos_parallax"][res["choice"]]))) - degrees) < 0.01, name
    q, res = RS.solved_scene("general")
    assert R.accept(1, res["cos_parallax"][2], 1.0) and not R.accept(1, res["cos_parallax"][2], 10.0)


# ------------------------------------------------------------------ the census
def census():
    table = {}
    for name, args in SCENES.items():
        table[name] = np.bincount(RS.solved_scene(*args)[1]["codes"].reshape(-1), minlength=8).tolist()
    q, _, _ = code1_problem()
    table["zero fourth component"] = np.bincount(RS.solve(q)["codes"].reshape(-1), minlength=8).tolist()
    return table


def test_census_every_code_is_reached_and_the_table_is_the_committed_one():
    """How often CheckRT goes each way, per scene, over all hypotheses (codes 0 .. 7 of orbfe_enqueue_reconstruct_initial)."""
    table = census()
    reached = np.sum([v for v in table.values()], axis=0)
    assert (reached > 0).all(), reached
    assert table["behind"][2] > 0 and table["behind"][3] > 0 and table["still"][6] > 300 and table["still"][7] == 0 and table["zero fourth component"][1] == 2     # the two hypotheses that share R share the vanishing point
    assert table["planar forced F"][4] > 0 and table["planar forced F"][5] > 0
    assert table == json.load(open(CENSUS)), "regenerate with: python -m tests.test_reconstruct_model"


# ------------------------------------------------------------------ the C++ host form
def _run(exe, q, tmp_path):
    problem, result = str(tmp_path / "problem.bin"), str(tmp_path / "out.bin")
    RS.write_problem_file(q, problem)
    H.run(exe, problem, result)
    return RS.read_result_file(q, result)


def mirror_cases():
    cases = [(name, RS.scene(*args)) for name, args in SCENES.items()]
    cases += [("%d matches" % n, truncated("general" if n % 2 else "frontal", n)) for n in (1, 8, 63, 64, 65, 255, 256, 257)]
    cases += [("nGood %d" % n, ngood_problem(n)[0]) for n in (0, 1, 50, 51, 52)]
    cases += [("no winner", RS.fresh(RS.scene("general"), best=np.array([-1, -1], np.int32))), ("identical frames", RS.identical_frames(0)),
              ("identical frames by RH", RS.identical_frames(-1)), ("zero fourth component", code1_problem()[0]),
              ("all flags zero, F", RS.with_flags(RS.scene("general"), 0, 1)), ("all flags zero, H", RS.with_flags(RS.scene("frontal"), 0, 0))]
    cases += [("%s %s" % (w, f), bad_pair(w, f)[0]) for w in ("first", "last") for f in ("idx1 == -1", "idx1 == n1", "idx2 == -1", "idx2 == n2")]
    return cases


@pytest.mark.parametrize("build", H.BUILDS)
def test_cpp_host_form_equals_the_model_bit_for_bit(tmp_path, build):
    exe = H.build(tmp_path, "reconstruct_mirror", build)
    for what, q in mirror_cases():
        want = RS.Outputs.expected(q, RS.solve(q))
        got = _run(exe, q, tmp_path)
        for k in RS.Outputs.NAMES:
            a, b = _bits(getattr(got, k)), _bits(getattr(want, k))
            assert np.array_equal(a, b), "%s: %s differs at bytes %s" % (what, k, np.nonzero(a != b)[0][:8].tolist())
    # what the call refuses: nothing is written
    q = truncated("general", 65)
    K = q["K"]
    for change in (dict(pairs=q["pairs"][:0], inl_h=q["inl_h"][:0], inl_f=q["inl_f"][:0]), dict(sigma=F32(0)), dict(sigma=F32(-1)), dict(K=K * F32([0, 1, 1, 1])),
                   dict(K=K * F32([1, -1, 1, 1])), dict(min_triangulated=-1), dict(model=2), dict(model=-2)):
        r = RS.fresh(q, **change)
        got, blank = _run(exe, r, tmp_path), RS.Outputs(r)
        assert got.status[0] == R.ERR_INVALID
        for k in RS.Outputs.NAMES[:-1]:
            assert np.array_equal(_bits(getattr(got, k)), _bits(getattr(blank, k))), (change, k)
    # ReconstructAccept: F wants parallax > minParallax, H parallax >= minParallax; 2.0 stands for nGood == 0
    cos5 = float(RS.solved_scene("general")[1]["cos_parallax"][2])
    for model, cos, min_parallax, want in ((1, cos5, 1.0, 1), (1, cos5, 10.0, 0), (0, cos5, 1.0, 1), (1, 2.0, 0.0, 0), (0, 2.0, 0.0, 1), (0, 1.0, 0.0, 1), (1, 1.0, 0.0, 0)):
        r = H.run(exe, "accept", str(model), repr(cos), repr(min_parallax))
        assert int(r.stdout) == want == int(R.accept(model, F32(cos), min_parallax)), (model, cos, min_parallax, r.stdout, r.stderr[-500:])


# ------------------------------------------------------------------ exports and refusals
def test_the_library_exports_both_calls_and_refuses_what_the_arguments_alone_show():
    """Without a device there is no context, and a NULL context is refused too -- so the refusals are told apart by the message."""
    from orbslam2_amd import api
    L = api.load()
    for name in NAMES:
        assert name in api.EXPORTS
        getattr(L, name)  # AttributeError: the symbol is not exported
    assert callable(api.Context.enqueue_reconstruct_initial) and callable(api.Context.reconstruct_initial) and callable(api.reconstruct_accept)
    assert L.orbfe_abi_version() == 6
    inputs = ["d_keys1", "n1", "d_keys2", "n2", "d_pairs", "N", "d_H21", "d_F21", "d_score", "d_best", "d_inl_h", "d_inl_f", "K", "sigma"]
    outputs = ["d_model", "d_hyp_R", "d_hyp_t", "d_ngood", "d_cos", "d_result", "d_choice", "d_R21", "d_t21", "d_p3d", "d_tri", "d_codes"]
    K = (C.c_float * 4)(520, 520, 320, 240)
    good = dict({k: 8 for k in inputs + outputs if k.startswith("d_")}, n1=100, n2=120, N=50, K=K, sigma=1.0, min_parallax=1.0, min_triangulated=50, model=-1, d_status=8, ok=8)
    forms = {"enqueue": (L.orbfe_enqueue_reconstruct_initial, inputs + ["min_triangulated", "model"] + outputs + ["d_status", "stream"], "d_status"),
             "synchronous": (L.orbfe_reconstruct_initial, inputs + ["min_parallax", "min_triangulated", "model"] + outputs + ["ok"], "ok")}
    for form, (fn, order, last) in forms.items():
        def call(**kw):
            a = dict(good, stream=0, **kw)
            return fn(None, *[(a[k] or None) if k.startswith("d_") or k in ("ok", "stream") else a[k] for k in order]), L.orbfe_last_error(None).decode()

        refusals = [(dict(**{k: 0}), "null input") for k in inputs if k.startswith("d_")] + [(dict(K=None), "null input")]
        refusals += [(dict(**{k: 0}), "null output") for k in outputs[:-1] + [last]]
        refusals += [(dict(N=0), "N = 0 < 1"), (dict(N=-3), "< 1"), (dict(n1=-1), "negative count"), (dict(N=65536), "above its limit"), (dict(n2=(1 << 24) + 1), "above its limit"),
                     (dict(sigma=0.0), "sigma must be > 0"), (dict(sigma=float("nan")), "sigma must be > 0"), (dict(K=(C.c_float * 4)(0, 520, 320, 240)), "fx and fy must be > 0"),
                     (dict(K=(C.c_float * 4)(520, float("nan"), 320, 240)), "fx and fy must be > 0"), (dict(min_triangulated=-1), "min_triangulated = -1 < 0"),
                     (dict(model=2), "model = 2 outside -1 .. 1"), (dict(model=-2), "model = -2 outside -1 .. 1")]
        for kw, message in refusals:
            rc, err = call(**kw)
            assert rc == api.ERR_INVALID and message in err, (form, kw, rc, err)
        for kw in (dict(), dict(d_codes=0), dict(N=1, n1=0, n2=0), dict(N=65535, model=1, min_triangulated=0)):
            assert call(**kw) == (api.ERR_INVALID, "null context"), (form, kw)
    header = open(os.path.join(ROOT, "include", "orbfe.h")).read()
    assert all("int %s(" % n in header for n in NAMES)


if __name__ == "__main__":
    with open(CENSUS, "w") as f:
        json.dump(census(), f, indent=1)
        f.write("\n")
    print("wrote", CENSUS)
