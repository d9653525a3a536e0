"""tests/lba_model.py, the float64 model of orbfe_enqueue_local_bundle_adjustment, proved on the CPU: its Jacobians against central
differences, its Schur path against a dense solve of the full system, a noiseless scene back at the ground truth, round 2 against
scipy's least squares, one scene per restated quirk of the reference, and the classification margins of every scene of
tests/lba_scenes.py that tests/test_lba_device.py then compares exactly."""
import numpy as np
import pytest

from tests import lba_model as M
from tests import lba_scenes as S
from tests import pose_blocks_model as PB


def _one_edge(stereo, seed):
    rng = np.random.default_rng(seed)
    pose = np.concatenate([PB.quat_from_matrix(PB.rot(rng.uniform(-0.3, 0.3, 3)))[0], rng.uniform(-0.5, 0.5, 3)])
    X = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(4, 8)])
    obs = np.array([300.0, 200.0, 290.0 if stereo else 0.0])
    return pose, X, obs


def _error(pose, X, obs, stereo):
    R = PB.quat_to_matrix(pose)[None]
    return M.edge_errors(S.CAM, R, pose[None, 4:7], X[None], obs[None], np.array([stereo]))[0][0]


@pytest.mark.parametrize("stereo", [False, True])
def test_point_and_pose_jacobians_against_central_differences(stereo):
    for seed in range(5):
        pose, X, obs = _one_edge(stereo, seed)
        R = PB.quat_to_matrix(pose)[None]
        _, P = M.edge_errors(S.CAM, R, pose[None, 4:7], X[None], obs[None], np.array([stereo]))
        Ji, Jj = M.jacobians(S.CAM, R, P, np.array([stereo]))
        # the stereo edge rounds 1 / z to float inside the error: its difference quotient needs a step that the float's granularity
        # (1.5e-8 of 1 / z) does not dominate
        h, tol = (1e-3, 2e-3) if stereo else (1e-6, 2e-5)
        for c in range(3):
            d = np.zeros(3)
            d[c] = h
            num = (_error(pose, X + d, obs, stereo) - _error(pose, X - d, obs, stereo)) / (2 * h)
            assert np.abs(num - Ji[0][:, c]).max() < tol * max(1.0, np.abs(Ji[0]).max()), (seed, c)
        for c in range(6):
            d = np.zeros(6)
            d[c] = h
            num = (_error(PB.se3_mul(M.se3_exp(d), pose), X, obs, stereo) - _error(PB.se3_mul(M.se3_exp(-d), pose), X, obs, stereo)) / (2 * h)
            assert np.abs(num - Jj[0][:, c]).max() < tol * max(1.0, np.abs(Jj[0]).max()), (seed, c)
        if not stereo:
            assert (Ji[0][2] == 0).all() and (Jj[0][2] == 0).all()


def _problem(name):
    s = S.scene(name)
    p = M.build(s["kfs"], s["role"], s["Tcw"], s["row"], s["n_rows"], s["obs_off"], s["obs_kf"], s["obs_idx"], s["pos"], S.INV_SIGMA2, S.NLEVELS)
    return s, p


@pytest.mark.parametrize("robust", [True, False])
def test_schur_step_equals_a_dense_solve_of_the_full_system(robust):
    s, p = _problem("mixed")
    act = np.nonzero(p.valid)[0]
    lin = M.linearize(p, S.CAM, p.pose, p.X, act, robust)
    lam = M.lambda_init(p, lin)
    assert lam > 0
    xp, xl = M.solve(p, lin, lam)
    K, N = len(lin.free), p.n_pts
    H, b = np.zeros((6 * K + 3 * N, 6 * K + 3 * N)), np.zeros(6 * K + 3 * N)
    for r, k in enumerate(lin.free):
        H[6 * r:6 * r + 6, 6 * r:6 * r + 6] = lin.Hpp[k]
        b[6 * r:6 * r + 6] = lin.bp[k]
    for q in range(N):
        H[6 * K + 3 * q:6 * K + 3 * q + 3, 6 * K + 3 * q:6 * K + 3 * q + 3] = lin.Hll[q]
        b[6 * K + 3 * q:6 * K + 3 * q + 3] = lin.bl[q]
    for a in np.nonzero(lin.on_free)[0]:
        r, q = lin.red[int(p.e_kf[act[a]])], int(p.e_pt[act[a]])
        H[6 * r:6 * r + 6, 6 * K + 3 * q:6 * K + 3 * q + 3] += lin.Hpl[a]
        H[6 * K + 3 * q:6 * K + 3 * q + 3, 6 * r:6 * r + 6] += lin.Hpl[a].T
    x = np.linalg.solve(H + lam * np.eye(len(b)), b)
    assert np.abs(x[:6 * K] - xp.reshape(-1)).max() < 1e-9 * np.abs(x).max()
    assert np.abs(x[6 * K:] - xl.reshape(-1)).max() < 1e-9 * np.abs(x).max()


def test_dense_ldlt_failure_rule():
    rng = np.random.default_rng(0)
    A = rng.normal(size=(12, 12))
    A = A @ A.T + np.eye(12)
    b = rng.normal(size=12)
    assert np.abs(M.ldlt_solve(A, b) - np.linalg.solve(A, b)).max() < 1e-12
    A[0, 0] = 0.0                                                       # an exactly zero pivot fails ...
    assert M.ldlt_solve(A, b) is None
    assert np.isnan(M.ldlt_solve(np.full((3, 3), np.nan), np.ones(3))).all()   # ... a NaN pivot does not
    assert len(M.ldlt_solve(np.zeros((0, 0)), np.zeros(0))) == 0


def test_noiseless_perturbed_scene_returns_to_ground_truth():
    s = S.make(seed=31, roles=[S.L, S.F, S.L, S.H, S.L, S.F], noise=0.0, outliers=0.0)
    r = S.run_model(s)
    assert r["status"] == 0 and len(r["erase"]) == 0 and (r["edge_code"] == 0).all()
    # the observations are floats (3e-5 px), the fixed poses floats of the ground truth: 1e-5 m is their size at 10 m
    assert np.abs(r["X"] - s["Xgt"]).max() < 2e-4
    for k in np.nonzero(s["role"] == S.L)[0]:
        assert np.abs(PB.pose_to_matrix(r["poses"][k]) - s["Tgt"][k]).max() < 5e-5, k
    assert r["info"]["chi2_second"] < 1e-3 < r["info"]["chi2_start"]


def test_round_two_continued_agrees_with_scipy_least_squares():
    """optimize(10) run on to convergence is the linear least-squares minimum over the surviving edges with the fixed and held
    keyframes as the gauge."""
    from scipy.optimize import least_squares
    s = S.scene("mixed")
    r = S.run_model(s, iterations=(5, 200))
    p = M.build(s["kfs"], s["role"], s["Tcw"], s["row"], s["n_rows"], s["obs_off"], s["obs_kf"], s["obs_idx"], s["pos"], S.INV_SIGMA2, S.NLEVELS)
    act = np.nonzero(p.valid & ((r["edge_code"] & M.CODE_LEVEL1) == 0))[0]
    free = np.nonzero(s["role"] == S.L)[0]
    pts = np.unique(p.e_pt[act])

    def unpack(v):
        pose, X = r["poses"].copy(), r["X"].copy()
        for i, k in enumerate(free):
            pose[k] = PB.se3_mul(M.se3_exp(v[6 * i:6 * i + 6]), r["poses"][k])
        X[pts] = r["X"][pts] + v[6 * len(free):].reshape(-1, 3)
        return pose, X

    def residuals(v):
        pose, X = unpack(v)
        e, _, _, _ = M.errors(p, S.CAM, pose, X, act)
        return (e * np.sqrt(p.info[act])[:, None]).reshape(-1)
    v0 = np.zeros(6 * len(free) + 3 * len(pts))
    sol = least_squares(residuals, v0, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
    assert abs(sol.cost * 2 - r["info"]["chi2_second"]) < 1e-6 * r["info"]["chi2_second"]
    assert np.abs(sol.x).max() < 1e-5                                  # the model's minimum is scipy's


def test_quirk_a_chi2_is_the_last_evaluation():
    """A level-1 edge keeps round 1's chi2 in the last test; recomputing it at the final estimates (the "fix") changes the values, and
    `stale` ends round 2 on rejected trials."""
    ref = S.model("mixed")
    fixed = S.run_model(S.scene("mixed"), quirks=M.ALL_QUIRKS - {"stale_chi2"})
    lvl1 = (ref["edge_code"] & M.CODE_LEVEL1) != 0
    assert lvl1.any() and (ref["edge_chi2"][lvl1] != fixed["edge_chi2"][lvl1]).all()
    assert np.abs(ref["edge_chi2"][lvl1] / fixed["edge_chi2"][lvl1] - 1).max() > 1e-3
    assert S.model("stale")["last_rejected"] == [False, True]


def test_quirk_b_depth_is_read_at_the_current_estimates():
    """`behind`: edges whose chi2 is small and whose point lies behind the camera are flagged by isDepthPositive alone."""
    s, ref = S.scene("behind"), S.model("behind")
    j = np.arange(s["obs_off"][40], s["obs_off"][43])
    assert len(j) == 9 and (ref["edge_chi2"][j] < 5.0).all() and (ref["edge_code"][j] == 3).all()
    listed = set(map(tuple, ref["erase"].tolist()))
    assert all((int(s["obs_kf"][i]), int(q)) in listed for i, q in zip(j, np.repeat([40, 41, 42], 3)))
    n_mono_erased = sum(1 for i in np.nonzero(ref["edge_code"] & M.CODE_ERASE)[0] if s["kfs"][s["obs_kf"][i]][1][s["obs_idx"][i]] < 0)
    first = [i for i in np.nonzero(ref["edge_code"] & M.CODE_ERASE)[0] if s["kfs"][s["obs_kf"][i]][1][s["obs_idx"][i]] < 0]
    assert [tuple(e) for e in ref["erase"][:n_mono_erased].tolist()] == [(int(s["obs_kf"][i]), int(np.searchsorted(s["obs_off"], i, side="right") - 1)) for i in first]


def test_quirk_c_a_vertex_without_a_level_0_edge_is_not_part_of_round_two():
    s, ref = S.scene("orphans"), S.model("orphans")
    assert ref["reduced"] == [24, 18]                                  # keyframe 5 gives the reduced system no block in round 2
    p = M.build(s["kfs"], s["role"], s["Tcw"], s["row"], s["n_rows"], s["obs_off"], s["obs_kf"], s["obs_idx"], s["pos"], S.INV_SIGMA2, S.NLEVELS)
    r1 = S.run_model(s, iterations=(5, 0))
    assert np.array_equal(ref["poses"][5], r1["poses"][5]) and np.array_equal(ref["X"][30:], r1["X"][30:])   # estimates kept, bit for bit
    assert not np.array_equal(ref["poses"][0], r1["poses"][0])
    fixed = S.run_model(s, quirks=M.ALL_QUIRKS - {"orphans"})
    assert fixed["reduced"] == [24, 24]


def test_quirk_d_a_held_keyframe_is_rewritten_through_the_quaternion():
    s, ref = S.scene("mixed"), S.model("mixed")
    k = 3
    assert s["role"][k] == S.H and ref["rewritten"][k]
    assert ref["Tcw"][k].tobytes() == PB.pose_to_cv(PB.pose_from_cv(s["Tcw"][k])[0]).reshape(16).tobytes()
    assert ref["Tcw"][k].tobytes() != s["Tcw"][k].tobytes()           # not left alone: the float row changes in its last digits
    fixed = S.run_model(s, quirks=M.ALL_QUIRKS - {"held_rewrite"})
    assert fixed["Tcw"][k].tobytes() == s["Tcw"][k].tobytes() and not fixed["rewritten"][k]


def test_quirk_e_fixed_and_skipped_rows_keep_their_bits():
    s, ref = S.scene("skip"), S.model("skip")
    for k in np.nonzero((s["role"] == S.F) | (s["role"] == S.S))[0]:
        assert ref["Tcw"][k].tobytes() == s["Tcw"][k].tobytes() and not ref["rewritten"][k]
    fixed = S.run_model(s, quirks=M.ALL_QUIRKS - {"fixed_bits"})
    assert any(fixed["Tcw"][k].tobytes() != s["Tcw"][k].tobytes() for k in np.nonzero(s["role"] == S.F)[0])
    s, ref = S.scene("rows"), S.model("rows")
    other = np.ones(s["n_rows"], bool)
    other[s["row"]] = False
    assert other.sum() == 17 and ref["pos"][other].tobytes() == s["pos"][other].tobytes()


@pytest.mark.parametrize("name", S.DEVICE_SCENES)
def test_every_scene_keeps_its_margins_and_its_gauge(name):
    s, ref = S.scene(name), S.model(name)
    if name in S.EMPTY:
        assert ref["status"] == 0 and ref["info"]["n_mono"] + ref["info"]["n_stereo"] == 0
        return
    assert ref["status"] == (M.ERR_INVALID if name in S.FAULTY else 0)
    for m in ref["margins"]:
        assert m["chi"] >= 0.01 and m["depth"] >= S.DEPTH_MARGIN, (name, m)
    assert len(ref["margins"]) == 2
    assert np.abs(s["pos"]).max() < 16 and np.abs(s["Tcw"]).max() < 16
    p = M.build(s["kfs"], s["role"], s["Tcw"], s["row"], s["n_rows"], s["obs_off"], s["obs_kf"], s["obs_idx"], s["pos"], S.INV_SIGMA2, S.NLEVELS)
    gauge = [k for k in range(len(s["role"])) if s["role"][k] in (S.H, S.F)]
    stereo = [k for k in gauge if (p.valid & p.stereo & (p.e_kf == k)).any()]
    mono = [k for k in gauge if (p.valid & (p.e_kf == k)).any()]
    assert stereo or len(mono) >= 2, name


@pytest.mark.parametrize("n", [63, 64, 65])
def test_the_batch_boundary_scenes_are_what_their_names_say(n):
    """views_n: one list of n entries, a free keyframe's edge last, all at level 0 in both rounds.  kf_edges_n: free keyframe 2 has n
    edges, all at level 0 in both rounds."""
    s, ref = S.scene("views_%d" % n), S.model("views_%d" % n)
    ln = np.diff(s["obs_off"])
    q = int(np.argmax(ln))
    a, b = s["obs_off"][q], s["obs_off"][q + 1]
    assert ln.max() == n and np.sort(ln)[-2] <= 4 and s["role"][s["obs_kf"][b - 1]] == S.L and (ref["edge_code"][a:b] == 0).all()
    assert len(set(s["obs_kf"][a:b].tolist())) == n
    s, ref = S.scene("kf_edges_%d" % n), S.model("kf_edges_%d" % n)
    on = s["obs_kf"] == 2
    assert s["role"][2] == S.L and on.sum() == n and (ref["edge_code"][on] == 0).all()


def test_faulty_scenes_equal_the_model_without_those_edges():
    clean = S.scene("rows")
    for name in S.FAULTY:
        s, ref = S.scene(name), S.model(name)
        if name == "faulty_descending":                                 # the clean scene behind one faulty point that owns nothing
            want = S.model("rows")
            assert np.array_equal(want["edge_code"], ref["edge_code"]) and want["Tcw"].tobytes() == ref["Tcw"].tobytes()
            assert want["pos"].tobytes() == ref["pos"].tobytes() and want["iterations"] == ref["iterations"]
            assert np.array_equal(want["erase"] + [0, 1], ref["erase"]) and ref["info"]["n_points"] == want["info"]["n_points"]
            continue
        faulty = ref["edge_code"] == M.CODE_FAULTY
        if name == "faulty_offset":
            faulty[:clean["obs_off"][1]] = True
            faulty[clean["obs_off"][-2]:] = True
        assert faulty.any(), name
        keep = ~faulty
        t = S.scene("rows")
        pt = np.searchsorted(clean["obs_off"], np.arange(len(keep)), side="right") - 1
        t["obs_kf"], t["obs_idx"] = clean["obs_kf"][keep], clean["obs_idx"][keep]
        t["obs_off"] = np.concatenate([[0], np.cumsum(np.bincount(pt[keep], minlength=len(clean["obs_off"]) - 1))]).astype(np.int32)
        if name == "faulty_role":
            t["role"] = s["role"].copy()
            t["role"][4] = S.S
        if name == "faulty_octave":
            t["kfs"] = s["kfs"]
        want = S.run_model(t)
        assert np.array_equal(want["edge_code"], ref["edge_code"][keep]), name
        assert want["Tcw"].tobytes() == ref["Tcw"].tobytes(), name
        rows = np.ones(s["n_rows"], bool)
        if name == "faulty_row":
            rows[clean["row"][[2, 11]]] = False                        # the model without the edges still rewrites the rows it names
        assert want["pos"][rows].tobytes() == ref["pos"][rows].tobytes(), name
        assert want["iterations"] == ref["iterations"] and want["trials"] == ref["trials"], name
