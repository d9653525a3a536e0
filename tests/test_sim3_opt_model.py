"""The float64 model of orbfe_enqueue_optimize_sim3 (tests/sim3_opt_model.py) proven on the CPU before a GPU sees it: the Sim3 algebra
against matrix exponentials and 4 x 4 products, the numeric Jacobian against the analytic derivative of the same error, the solver
against the truth of a noiseless scene and against scipy's least_squares on the same robust cost, and the call's bookkeeping (merge
with prior12, invalid slots, the early return, fix_scale, the status) on the scenes of tests/sim3_opt_scenes.py -- the very scenes and
block cases tests/test_sim3_blocks.py and tests/test_sim3_opt_device.py compare the kernels with the model on.
"""
import ctypes as C
import math
import os

import numpy as np

from tests import sim3_opt_model as M
from tests import sim3_opt_scenes as S

NAMES = ["orbfe_enqueue_optimize_sim3", "orbfe_optimize_sim3"]


def _generator(u):
    """The 4 x 4 generator of the similarity group for u = (omega, upsilon, sigma)."""
    w = u[:3]
    A = np.zeros((4, 4))
    A[:3, :3] = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) + u[6] * np.eye(3)
    A[:3, 3] = u[3:6]
    return A


def test_the_library_exports_both_calls():
    from orbslam2_amd import api
    L = api.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "orbfe.h")).read()
    for name in NAMES:
        assert name in api.EXPORTS and ("int %s(" % name) in header
        fn = getattr(L, name)  # AttributeError: the symbol is not exported
        args = [0 if t is C.c_int else 0.0 if t is C.c_float else None for t in fn.argtypes]
        assert fn(*args) == api.ERR_INVALID, name
    for m in ("enqueue_optimize_sim3", "optimize_sim3"):
        assert callable(getattr(api.Context, m))
    assert C.sizeof(api.Sim3OptParams) == 16
    assert "#define ORBFE_SIM3_OPT_LDS_SLOTS %d" % S.LDS_SLOTS in header


def test_sim3_of_rotation_translation_scale_takes_every_quaternion_branch():
    from tests.pose_blocks_model import quat_branch
    seen = set()
    for name, R, t, s, want in S.rts_cases():
        assert quat_branch(R) == want, name
        seen.add(want)
        Sm = M.sim3(R, t, s)
        if name != "not_orthonormal":
            assert abs(np.linalg.norm(Sm[0]) - 1) < 1e-14, name
            assert np.abs(M.quat_matrix(Sm[0]) - R).max() < 1e-14, name
        else:
            assert abs(np.linalg.norm(Sm[0]) - 1) > 1e-13   # Quaterniond(R) is not normalised, and the model keeps it so
        assert Sm[1] == tuple(t) and Sm[2] == s
    assert seen == {"trace", 0, 1, 2}


def test_exponential_equals_expm_in_all_four_branches():
    from scipy.linalg import expm
    seen = set()
    for name, u, branch, kind in S.exp_cases():
        assert M.exp_branch(u) == branch, name
        if kind != "expm":
            continue
        seen.add(branch)
        q, t, s = M.sim3_exp(u)
        got = M.sim3_matrix((tuple(np.array(q) / np.linalg.norm(q)), t, s))
        assert np.abs(got - expm(_generator(u))).max() < 1e-12, name
    assert seen == {(True, True), (True, False), (False, True), (False, False)}
    # next to the thresholds the branches are approximations: the small-theta form misses half of Omega^2 upsilon-scale terms
    by = {c[0]: c for c in S.exp_cases()}
    u = by["theta_below"][1]
    assert np.abs(M.sim3_matrix(M.sim3_exp(u)) - expm(_generator(u))).max() > 1e-11
    # R = I + Omega + Omega^2 goes to Quaterniond(R) as it is: the quaternion is not unit
    assert abs(np.linalg.norm(M.sim3_exp(u)[0]) - 1) > 1e-11


def test_product_inverse_and_map_equal_the_4x4_similarities():
    """On unit quaternions (the cases of the device test carry a norm defect of 1e-3, as g2o's do after many products; Eigen's
    rotation formula is the rotation only at unit norm, so the matrix identities are checked on the normalised copies)."""
    def unit(v):
        v = np.array(v, np.float64)
        v[:4] /= np.linalg.norm(v[:4])
        return M.unpack(v)
    for name, a, b, p in S.sim3_cases():
        A, B = unit(a), unit(b)
        assert np.abs(M.sim3_matrix(M.sim3_mul(A, B)) - M.sim3_matrix(A) @ M.sim3_matrix(B)).max() < 1e-13, name
        assert np.abs(M.sim3_matrix(M.sim3_mul(A, M.sim3_inverse(A))) - np.eye(4)).max() < 1e-13, name      # S * S.inverse() is the identity
        assert np.abs(M.sim3_matrix(M.sim3_inverse(A)) - np.linalg.inv(M.sim3_matrix(A))).max() < 1e-13, name
        assert np.abs(np.array(M.sim3_map(A, *p)) - (M.sim3_matrix(A) @ np.append(p, 1))[:3]).max() < 1e-13, name
        assert abs(np.linalg.norm(a[:4]) - 1) > 1e-6 or abs(np.linalg.norm(b[:4]) - 1) > 1e-6


def test_ldlt7_solves_detects_indefinite_and_reaches_every_exchange():
    seen = set()
    for name, H, b, lam in S.ldlt7_cases():
        x, positive, piv = M.ldlt_solve(H, b, lam)
        seen |= {(k, p) for k, p in piv if p != k}
        if name == "indefinite":
            assert not positive and x is None
            continue
        assert positive, name
        if name.startswith("swap_"):
            K, Cc = int(name[5]), int(name[7])
            assert piv[K] == (K, Cc) and all(p == k for k, p in piv[:K]), (name, piv)
        if name == "zero_row_col":
            assert x[2] == 0.0
            continue
        Hl = np.asarray(H, np.float64) + lam * np.eye(7)
        ref = np.linalg.solve(Hl, b)
        assert np.abs(x - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max()) * np.linalg.cond(Hl) * 1e-3 + 1e-12, name
        if name == "fix_scale":
            assert x[6] == 0.0
    assert seen == {(k, c) for k in range(6) for c in range(k + 1, 7)}


def _analytic_jacobians(T, est):
    """d e / d update at update = 0 for both edges: with p = S.map(P2), exp(u) S maps P2 to p + omega x p + upsilon + sigma p; with
    (exp(u) S)^-1 = S^-1 exp(-u), the inverse edge sees S^-1 applied to P1 - omega x P1 - upsilon - sigma P1."""
    fx, fy, _, _ = S.CAM
    def dproj(p):
        return np.array([[fx / p[2], 0, -fx * p[0] / p[2] ** 2], [0, fy / p[2], -fy * p[1] / p[2] ** 2]])
    def skew(v):
        return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    inv = M.sim3_inverse(est)
    Ainv = M.sim3_matrix(inv)[:3, :3]
    J12, J21 = [], []
    for k in range(len(T)):
        p = np.array(M.sim3_map(est, *T.P2[k]))
        J12.append(-dproj(p) @ np.concatenate([-skew(p), np.eye(3), p[:, None]], 1))
        P1 = T.P1[k]
        q = np.array(M.sim3_map(inv, *P1))
        J21.append(dproj(q) @ Ainv @ np.concatenate([-skew(P1), np.eye(3), P1[:, None]], 1))
    return np.array(J12), np.array(J21)


def test_numeric_jacobian_agrees_with_the_analytic_derivative_to_the_quotients_noise():
    """The central difference over +-1e-9 divides the rounding errors of two error evaluations by 2e-9.  One evaluation makes a few
    dozen roundings, each relative to the pixel coordinate it ends in (|obs| + |proj| < 1500) or, through the point in camera
    coordinates, to fx (1 + (x/z)^2 + (y/z)^2): 48 roundings of 2^-53 on 2000 px are 1.1e-11 px, which the quotient turns into
    5e-3; the truncation error (third derivative times 1e-18) is far below.  Entries of J are 1e2 to 1e4."""
    cs, _ = S.eval_refs()
    worst = 0.0
    for name, T, est, fix in cs:
        _, _, _, _, J12, J21 = M.evaluate(T, est, fix, S.CAM, 3.0)
        A12, A21 = _analytic_jacobians(T, est)
        if fix:
            assert (J12[:, :, 6] == 0).all() and (J21[:, :, 6] == 0).all(), name   # exactly zero, not small
            A12[:, :, 6] = 0; A21[:, :, 6] = 0
        err = max(np.abs(J12 - A12).max(), np.abs(J21 - A21).max())
        worst = max(worst, err)
        assert err < 5e-3, (name, err)
        assert np.abs(A12).max() > 100
    print("numeric - analytic Jacobian: largest difference %.3e" % worst)


def test_a_noiseless_scene_recovers_the_true_sim3():
    """Inputs are float32: a coordinate of 20 m carries 1e-6 m, an observation 4e-5 px; the recovered Sim3 is within 1e-5 of the truth."""
    s, r = S.scene("noiseless"), S.model("noiseless")
    Rt, tt, st = s["truth"]
    q, t, sc = M.unpack(r["S12"])
    assert r["n_inliers"] == 40 and r["status"] == 0
    assert np.abs(M.quat_matrix(np.array(q) / np.linalg.norm(q)) - Rt).max() < 1e-5
    assert np.abs(np.array(t) - tt).max() < 1e-5 and abs(sc - st) < 1e-5


def _robust_cost_residuals(T, fix_scale, s_fixed):
    from scipy.spatial.transform import Rotation
    delta = float(np.float32(math.sqrt(S.TH2)))
    act = T.active

    def resid(p):
        sc = s_fixed if fix_scale else math.exp(p[6])
        R = Rotation.from_rotvec(p[:3]).as_matrix()
        fx, fy, cx, cy = S.CAM
        a = (sc * (T.P2[act] @ R.T) + p[3:6])
        b = ((T.P1[act] - p[3:6]) @ R) / sc
        out = []
        for X, obs, info in ((a, T.obs1[act], T.info1[act]), (b, T.obs2[act], T.info2[act])):
            e = np.stack([obs[:, 0] - (fx * X[:, 0] / X[:, 2] + cx), obs[:, 1] - (fy * X[:, 1] / X[:, 2] + cy)], 1)
            chi = info * (e ** 2).sum(1)
            rho = np.where(chi <= delta * delta, chi, 2 * np.sqrt(chi) * delta - delta * delta)
            out.append((e * np.sqrt(info)[:, None] * np.sqrt(rho / np.maximum(chi, 1e-300))[:, None]).reshape(-1))
        return np.concatenate(out)
    return resid


def test_the_final_estimate_is_a_least_squares_optimum_of_the_robust_cost():
    """scipy's least_squares on the same Huber cost over the second round's edges, started at the model's estimate, must not find a
    noticeably smaller cost (the bounds of tests/test_pose.py's check of the pose)."""
    from scipy.optimize import least_squares
    from scipy.spatial.transform import Rotation
    for name in ("clean", "outliers", "fix_scale", "corr300"):
        s, r = S.scene(name), S.model(name)
        q, t, sc = M.unpack(r["S12"])
        resid = _robust_cost_residuals(r["table"], bool(s["fix_scale"]), float(s["s12"]))
        p0 = np.concatenate([Rotation.from_matrix(M.quat_matrix(np.array(q) / np.linalg.norm(q))).as_rotvec(), t, [math.log(sc)]])
        c0 = float((resid(p0) ** 2).sum())
        sol = least_squares(resid, p0, method="lm", xtol=1e-14, ftol=1e-14)
        c1 = float((sol.fun ** 2).sum())
        assert c1 <= c0 * (1 + 1e-9), name
        assert c0 - c1 <= 2e-3 * c0, (name, c0, c1)
        assert np.abs(sol.x - p0).max() < 2e-4, (name, np.abs(sol.x - p0).max())


def test_fix_scale_keeps_the_scale_exactly():
    s, r = S.scene("fix_scale"), S.model("fix_scale")
    assert r["n_inliers"] == 37 and r["S12"][7] == float(s["s12"]) == 1.0
    assert np.abs(r["S12"][4:7] - s["t12"]).max() > 1e-3   # the rest moved


def test_the_early_return_leaves_the_input_and_clears_exactly_the_bad_entries():
    s, r = S.scene("early"), S.model("early")
    S_in = M.sim3(s["R12"].astype(np.float64), s["t12"].astype(np.float64), float(s["s12"]))
    assert r["n_inliers"] == 0 and r["chi_second"] is None and r["iterations"][1] == 0
    assert np.array_equal(r["S12"], M.pack(S_in))
    bad = (r["chi_first"] > S.TH2).any(1)
    assert bad.sum() == 4 and set(s["slots1"][bad]) == set(s["slots1"][s["outliers"]])
    want = s["match12"].copy()
    want[s["slots1"][bad]] = -1
    assert np.array_equal(r["match12"], want) and (r["match12"] >= 0).sum() == 8


def test_an_invalid_slot_keeps_its_entry_and_is_not_counted():
    s, r = S.scene("invalid_slots"), S.model("invalid_slots")
    held = s["slots1"][[3, 7, 20]]
    assert r["n_corr"] == 37 and not set(held) & set(r["slots"])
    assert np.array_equal(r["match12"][held], s["match12"][held]) and (s["match12"][held] >= 0).all()
    assert r["n_inliers"] == 35 and (r["match12"] >= 0).sum() == 35 + 3


def test_prior12_is_merged_on_the_slots():
    s, r = S.scene("prior"), S.model("prior")
    assert (s["prior12"] >= 0).sum() == 14 and (s["match12"] >= 0).sum() == 26 and (s["prior12"] == -5).sum() == 2
    assert not ((s["prior12"] >= 0) & (s["match12"] >= 0)).any()
    merged = np.where(s["prior12"] >= 0, s["prior12"], s["match12"])
    assert r["n_corr"] == 40 and np.array_equal(r["slots"], s["slots1"])
    kept = r["match12"] >= 0
    assert np.array_equal(r["match12"][kept], merged[kept]) and kept.sum() == r["n_inliers"] == 36
    assert kept[s["prior12"] >= 0].any() and kept[s["match12"] >= 0].any()


def test_out_of_range_entries_set_the_status_and_harm_no_other_row():
    for bad, good in (("bad_match_high", None), ("bad_match_low", None), ("bad_octave1", None), ("bad_octave2", None)):
        s, r = S.scene(bad), S.model(bad)
        k = 5 if "match" in bad else 9
        assert r["status"] == M.ERR_INVALID and r["n_corr"] == 39 and r["match12"][s["slots1"][k]] == -1
        # the same scene without the faulty row's correspondence gives the same estimate: the row made no edge and touched nothing
        m2 = s["match12"].copy(); m2[s["slots1"][k]] = -1
        clean = S.run_model(s, match12=m2)
        assert clean["status"] == 0 and np.array_equal(clean["S12"], r["S12"]) and np.array_equal(clean["match12"], r["match12"])


def test_every_scene_keeps_its_distance_from_th2():
    for name in S.SPECS:
        assert S.margin(S.model(name)) > 0.01, name
    want = dict(clean=(40, 40, 0), outliers=(40, 34, 0), early=(12, 0, 0), none=(0, 0, 0), kf1_empty=(0, 0, 0), scratch_table=(64, 59, 0))
    for name, (nc, ni, st) in want.items():
        r = S.model(name)
        assert (r["n_corr"], r["n_inliers"], r["status"]) == (nc, ni, st), name
    # the paths the device tests name: clean -> more_iterations_clean, outliers -> more_iterations_outliers
    assert (S.model("clean")["chi_first"] <= S.TH2).all() and (S.model("outliers")["chi_first"] > S.TH2).any(1).sum() == 6
    assert len(S.scene("scratch_table")["keys1"]) > S.LDS_SLOTS
    assert set(S.scene("clean")["keys1"]["octave"][S.scene("clean")["slots1"]]) == set(range(8))
