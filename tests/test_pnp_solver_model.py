"""The model of the PnPsolver port (tests/pnp_solver_model.py) checked on the CPU, on the scenes of tests/pnp_solver_scenes.py.

A 4-point M is 8 x 12: the last four rows of Ut that EPnP reads span its null space, which basis of it comes out is decided by rounding
inside the Jacobi, and find_betas_approx_* are not invariant to that choice.  A 4-point hypothesis can therefore not be compared end to end
with an independent float64 path.  The exactness is carried by "one contract, implemented more than once, bit-equal"
(tests/test_pnp_solver_host.py, tests/test_pnp_ransac_device.py); the independent checks here are made STAGE BY STAGE against LAPACK
(numpy.linalg, float64), each stage fed the model's own inputs to it: the singular values of every SVD, the projector onto the last four
rows of Ut (the projector, not the rows), U V^T of estimate_R_and_t, the pseudo-inverse of CC, the three cvSolve solutions and every
qr_solve step against lstsq.  A stage instance is left out only when the float64 path finds its matrix's condition number above 1e8 or a
relative singular-value gap below 1e-8; at most 1 % per stage and scene.  Tolerances are the measured maxima times 8, one digit
(DESIGN.md section 4p lists the measurements).

End to end where it is well defined: Refine() on n >= 12 inliers against an independent float64 EPnP (eigh / svd / lstsq), and the first
event's refined pose against the scene's true inliers."""
import numpy as np
import pytest

from tests import pnp_solver_model as M
from tests import pnp_solver_scenes as S

STAGE_SCENES = ["clean", "outliers", "noisy", "n65"]
# measured maxima (this file's scenes) times 8, one digit; see _stage_errors for what each measures
# sv 2.1e-15 (relative to the largest), projector 3.1e-15, uvt 1.1e-14, cc_inv 5.9e-14 (relative to the largest entry), solve 3.3e-12 (the same),
# qr 8.5e-14 (relative to |A^+| |b|); nothing was left out
TOL = dict(sv=2e-14, projector=3e-14, uvt=9e-14, cc_inv=5e-13, solve=3e-11, qr=7e-13)


# ------------------------------------------------------------------ the literal walk
def literal_walk(N, counts, refine_ok, refined_n, min_inliers, max_its, step, max_calls=4096):
    """src/PnPsolver.cc:166-259 transcribed, iterate(step) called until bNoMore, over rows that hold per iteration mnInliersi, and per
    record holder whether Refine() succeeds and mnRefinedInliers.  One tuple per call: (return, bNoMore, nInliers, mnIterations, the
    record holder), return = the iteration of a refined pose, -2 for mBestTcw, -1 for an empty Mat.  The rows are all the solver has:
    where the loop asks for an iteration beyond them it ends as on exhaustion (orbslam2_amd/host/PnPsolver.h says so)."""
    mnIterations, mnBestInliers, best_k, out = 0, 0, -1, []
    for _ in range(max_calls):
        bNoMore, nInliers, ret = False, 0, None
        if N < min_inliers or max_its <= 0:
            out.append((-1, True, 0, mnIterations, best_k))
            break
        nCurrentIterations, ended = 0, False
        while mnIterations < max_its or nCurrentIterations < step:
            if mnIterations >= len(counts):
                ended = True
                break
            nCurrentIterations += 1
            mnIterations += 1
            k = mnIterations - 1
            if counts[k] >= min_inliers:
                if counts[k] > mnBestInliers:
                    mnBestInliers, best_k = int(counts[k]), k
                if refine_ok[best_k]:
                    nInliers, ret = int(refined_n[best_k]), k
                    break
        if ret is None:
            ret = -1
            if ended or mnIterations >= max_its:
                bNoMore = True
                if mnBestInliers >= min_inliers:
                    nInliers, ret = mnBestInliers, -2
        out.append((ret, bNoMore, nInliers, mnIterations, best_k))
        if bNoMore:
            break
    return out


def _replays():
    out = []
    for step in (1, 5, 300):
        out += [(40, 12, 20, step, [0] * 11 + [30], [1] * 12),                       # a success on the last iteration
                (40, 12, 20, step, [3, 25, 0, 22, 31, 0, 0, 26, 0, 0, 0, 0], [0] * 12),  # exhaustion with a best hypothesis
                (40, 12, 20, step, [3, 19, 0, 12, 7, 0, 0, 6, 0, 0, 0, 0], [1] * 12),     # exhaustion without one
                (40, 12, 20, step, [25, 0, 27, 0, 30, 24, 0, 0, 33, 0, 0, 29], [0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0]),   # records with and without a refinement
                (8, 0, 10, step, [0] * 5, [0] * 5),                                  # N < mRansacMinInliers
                (10, 1, 10, step, [10, 10, 9, 10, 10], [0] * 5),                     # N == mRansacMinInliers: the table gives 1, iterate(5) runs 5
                (40, 4, 20, step, [30, 0, 31, 0, 0, 32, 0, 0, 0, 0, 28, 0, 0, 0, 0, 0, 35, 0, 0, 0], [1] * 20)]   # calls after a success run on beyond mRansacMaxIts
    return out


REPLAYS = _replays()


def test_literal_walk_on_hand_written_rows():
    w = lambda r: literal_walk(r[0], r[4], r[5], r[4], r[2], r[1], r[3])
    last = [r for r in REPLAYS if r[4][-1] == 30]
    assert [[c[0] for c in w(r) if c[0] >= 0] for r in last] == [[11]] * 3
    # iterate(1): the `||` of :183 runs the first call up to mRansacMaxIts = 12; the next call finds the rows' end
    assert w(REPLAYS[0]) == [(11, False, 30, 12, 11), (-2, True, 30, 12, 11)]
    best = [r for r in REPLAYS if r[4][1] == 25]
    assert all(w(r)[-1][:3] == (-2, True, 31) for r in best)
    none = [r for r in REPLAYS if r[4][1] == 19]
    assert all(w(r)[-1][:3] == (-1, True, 0) for r in none)
    below = [r for r in REPLAYS if r[0] == 8]
    assert all(w(r) == [(-1, True, 0, 0, -1)] for r in below)
    at_min = [r for r in REPLAYS if r[0] == 10]
    assert [w(r)[-1][3] for r in at_min] == [1, 5, 5]                     # iterate(1) stops at mRansacMaxIts = 1, iterate(5) and (300) run the five rows
    assert all(w(r)[-1][:3] == (-2, True, 10) for r in at_min)
    after = [r for r in REPLAYS if r[1] == 4]
    assert [[c[0] for c in w(r) if c[0] >= 0] for r in after] == [[0, 2], [0, 2, 5, 10], [0, 2, 5, 10, 16]]   # a call after a success runs nIterations more, beyond mRansacMaxIts = 4
    mixed = [r for r in REPLAYS if r[5][2] == 1 and r[5][0] == 0]
    assert [[c[0] for c in w(r) if c[0] >= 0] for r in mixed] == [[2, 8, 11]] * 3          # 4 and 5 follow a failed record; 11 returns record 8's pose again


def test_iteration_table_keeps_the_reference_quirks():
    t = M.its_table(200, 0.99, 10, 300, 0.5)
    assert (t[:10] == 0).all() and t[10] == 1                            # N < mRansacMinInliers; N == mRansacMinInliers
    assert t[40] == 35 and t[200] == 35                                   # pow(epsilon, 3), not 4: ceil(log(0.01) / log(1 - 0.125))
    assert M.min_inliers_for(41, 10, 0.5) == 20 and M.min_inliers_for(19, 10, 0.5) == 10   # the int truncation of N * epsilon
    assert t[11] == M.iterations_for(11, 0.99, 10, 300, 0.5) == 4         # the float epsilon bump to 10 / 11: ceil(3.31)
    assert M.its_table(12, 0.99, 4, 300, 0.1)[4] == 1 and (M.its_table(12, 0.99, 2, 300, 0.1)[:4] == 0).all()   # the minimal set bounds it
    assert M.iterations_for(100, 0.99, 4, 300, 0.05) == 300               # the clamp


def test_the_package_table_equals_the_model_table():
    """orbslam2_amd.api.pnp_iteration_table is what a Python caller uploads as d_its_for_n."""
    from orbslam2_amd import api
    assert np.array_equal(api.pnp_iteration_table(400), M.its_table(400, 0.99, 10, 300, 0.5))
    for prob, mn, its, eps in ((0.99, 10, 300, 0.5), (0.99, 4, 300, 0.1), (0.999, 8, 300, 0.4), (0.99, 10, 300, 0.3), (0.5, 20, 50, 0.9), (0.99, 2, 7, 0.0), (0.99, 10, 300, 1.0)):
        assert np.array_equal(api.pnp_iteration_table(300, prob, mn, its, eps), M.its_table(300, prob, mn, its, eps)), (prob, mn, its, eps)


def test_draw_sets_follow_the_swap_with_back_and_pop():
    rng = np.random.default_rng(5)
    for N in (4, 5, 7, 40):
        for _ in range(50):
            ids = [int(i) for i in rng.choice(N, 4, replace=False)]
            assert M.draw_set(S.raw_for(ids, N), N) == ids
    assert M.draw_set([0, 0, 0, 0], 6) == [0, 5, 4, 3]                    # position 0 holds the back after every draw
    assert M.draw_set([M.RAND_MAX] * 4, 6) == [5, 4, 3, 2]


def test_scenes_have_the_properties_they_were_built_for():
    m = S.model("last_record")
    assert S.records(m) == [11] and m["events"][:m["n_events"]].tolist() == [11] and m["exhausted"] == 11
    m = S.model("many_records")
    assert len(S.records(m)) > 4, S.records(m)
    m = S.model("degenerate")
    assert (m["hyp"]["Rcw"][:2].view(np.uint32) == M.NAN_BITS).all() and (m["hyp"]["n_inliers"][:2] == 0).all() and m["n_events"] > 0
    m = S.model("hbm")
    assert m["n_corr"] == S.LDS_SLOTS + 1 and S.records(m) == [0, 2] and m["n_events"] == 3
    m = S.model("below_min")
    assert m["n_its"] == 0 and m["exhausted"] == -1 and not m["hyp"]["n_inliers"].any()
    m = S.model("at_min")
    assert m["n_corr"] == 10 and S.scene("at_min")["its_for_n"][10] == 1 and m["n_its"] == 5 and m["n_events"] == 0 and m["exhausted"] >= 0
    m = S.model("n4")
    assert m["n_corr"] == 4 and m["n_its"] == 5
    m = S.model("invalid_points")
    assert m["n_corr"] == 37 and m["status"] == 0
    for name in ("n65", "n70"):
        m = S.model(name)
        N = m["n_corr"]
        assert N == int(name[1:]) and not (m["bits"][:, N >> 5] >> np.uint32(N & 31)).any()


# ------------------------------------------------------------------ stage by stage against LAPACK
def _gap_ok(w, i):
    """The relative gap between singular values i - 1 and i (descending) of the float64 path."""
    return (w[i - 1] - w[i]) > 1e-8 * w[0]


def _stage_errors(st):
    """{stage: [(error, skipped)]} of one compute_pose, every stage fed the model's own input to it."""
    e = {k: [] for k in TOL}
    A = np.array(st["pw0tpw0"])
    e["sv"].append((np.abs(np.array(st["dc"]) - np.linalg.svd(A, compute_uv=False)).max() / max(np.linalg.norm(A, 2), 1e-300), False))
    A = np.array(st["mtm"])
    w_ref = np.linalg.svd(A, compute_uv=False)
    e["sv"].append((np.abs(np.array(st["d"]) - w_ref).max() / w_ref[0], False))
    ew, ev = np.linalg.eigh(A)                                            # ascending: the first four span what the last four rows of Ut span
    V4 = np.array(st["ut"])[8:]
    e["projector"].append((np.abs(V4.T @ V4 - ev[:, :4] @ ev[:, :4].T).max(), not _gap_ok(w_ref, 8)))
    A = np.array(st["cc"])
    cond = np.linalg.cond(A)
    ref = np.linalg.pinv(A)
    e["cc_inv"].append((np.abs(np.array(st["cc_inv"]) - ref).max() / np.abs(ref).max(), not cond < 1e8))
    e["sv"].append((np.abs(np.array(st["cc_w"]) - np.linalg.svd(A, compute_uv=False)).max() / np.linalg.norm(A, 2), False))
    for sv in st["solve"]:
        A, b = np.array(sv["A"]), np.array(st["rho"])
        ref = np.linalg.lstsq(A, b, rcond=None)[0]
        e["solve"].append((np.abs(np.array(sv["b"]) - ref).max() / np.abs(ref).max(), not np.linalg.cond(A) < 1e8))
        e["sv"].append((np.abs(np.array(sv["W"]) - np.linalg.svd(A, compute_uv=False)).max() / np.linalg.norm(A, 2), False))
    for ab in st["abt"]:
        A = np.array(ab["A"])
        u, w, vt = np.linalg.svd(A)
        e["uvt"].append((np.abs(np.array(ab["UVt"]) - u @ vt).max(), not (w[2] > 1e-8 * w[0])))
        e["sv"].append((np.abs(np.array(ab["W"]) - w).max() / w[0], False))
    for A0, b0, x in st["qr"]:
        A, b = np.array(A0).reshape(6, 4), np.array(b0)
        ref = np.linalg.lstsq(A, b, rcond=None)[0]
        scale = np.linalg.norm(b) / np.linalg.svd(A, compute_uv=False)[-1]     # |A^+| |b|: a converged step is all rounding, so not |ref|
        e["qr"].append((np.abs(np.array(x) - ref).max() / scale, not np.linalg.cond(A) < 1e8))
    return e


def stage_census(name):
    """{stage: (instances, skipped, largest error among the kept)} over every compute_pose of a scene: hypotheses and refinements."""
    tot = {k: [0, 0, 0.0] for k in TOL}
    for st in S.stages(name).values():
        for k, rows in _stage_errors(st).items():
            for err, skip in rows:
                tot[k][0] += 1
                if skip or not np.isfinite(err):
                    tot[k][1] += 1
                else:
                    tot[k][2] = max(tot[k][2], float(err))
    return {k: tuple(v) for k, v in tot.items()}


@pytest.mark.parametrize("name", STAGE_SCENES)
def test_every_stage_agrees_with_lapack(name):
    census = stage_census(name)
    for k, (n, skipped, worst) in census.items():
        print("%-9s %-10s %6d instances, %4d left out, largest difference %.2e (tolerance %.0e)" % (name, k, n, skipped, worst, TOL[k]))
    for k, (n, skipped, worst) in census.items():
        assert n > 0 and skipped * 100 <= n, (name, k, n, skipped)       # the cap: 1 % per stage and scene
        assert worst <= TOL[k], (name, k, worst)


# ------------------------------------------------------------------ end to end where it is well defined
def reference_epnp(P3D, P2D, cam):
    """An independent float64 EPnP for n >= 6 points in general position: control points by eigh, the one-dimensional null space of M by
    svd, the scale and the pose by a Procrustes fit; no Gauss-Newton (N = 1 with a single null vector is exact up to noise)."""
    fu, fv, uc, vc = cam
    X = np.asarray(P3D, np.float64)
    c0 = X.mean(0)
    w, v = np.linalg.eigh((X - c0).T @ (X - c0))
    cws = np.vstack([c0] + [c0 + np.sqrt(w[i] / len(X)) * v[:, i] for i in (2, 1, 0)])
    alphas = np.hstack([np.ones((len(X), 1)), X]) @ np.linalg.inv(np.hstack([np.ones((4, 1)), cws]))
    Mm = np.zeros((2 * len(X), 12))
    for j in range(4):
        Mm[0::2, 3 * j], Mm[0::2, 3 * j + 2] = alphas[:, j] * fu, alphas[:, j] * (uc - P2D[:, 0])
        Mm[1::2, 3 * j + 1], Mm[1::2, 3 * j + 2] = alphas[:, j] * fv, alphas[:, j] * (vc - P2D[:, 1])
    ccs = np.linalg.svd(Mm)[2][-1].reshape(4, 3)
    d = lambda c: np.array([np.linalg.norm(c[a] - c[b]) for a in range(4) for b in range(a + 1, 4)])
    ccs = ccs * (d(cws) @ d(ccs)) / (d(ccs) @ d(ccs))
    pcs = alphas @ ccs
    if pcs[0, 2] < 0:
        pcs = -pcs
    pc0, pw0 = pcs.mean(0), X.mean(0)
    u, _, vt = np.linalg.svd((pcs - pc0).T @ (X - pw0))
    R = u @ vt
    if np.linalg.det(R) < 0:
        R[2] = -R[2]
    return R, pc0 - R @ pw0


REFINE_SCENES = ["clean", "outliers", "n64", "n65", "last_record"]            # pixel noise of 0.5 at most: the reference has no Gauss-Newton
REFINE_TOL = dict(R=1e-2, t=2e-1)      # measured maxima over REFINE_SCENES, 1.2e-3 and 2.0e-2, times 8, one digit


def refine_census(name):
    """Per record holder with at least 12 inliers: (|R - R_ref| max, |t - t_ref| max, flags that differ beyond a relative 1e-3 of the gate)."""
    s, m = S.scene(name), S.model(name)
    tab = M.filter_frame(s)[0]
    cam = tuple(float(np.float32(v)) for v in s["cam"])
    rows = []
    for k in S.records(m):
        inl = M.unpack_bits(m["bits"][k], m["n_corr"])
        if inl.sum() < 12:
            continue
        R, t = reference_epnp(tab["P3D"][inl], tab["P2D"][inl].astype(np.float64), cam)
        T = m["refined"][k]["Tcw"].reshape(3, 4).astype(np.float64)
        Xc = tab["P3D"].astype(np.float64) @ R.T + t
        uv = np.stack([cam[2] + cam[0] * Xc[:, 0] / Xc[:, 2], cam[3] + cam[1] * Xc[:, 1] / Xc[:, 2]], 1)
        e2 = ((tab["P2D"] - uv) ** 2).sum(1)
        near = np.abs(e2 - tab["max_error"]) <= 1e-3 * tab["max_error"]
        flags = M.unpack_bits(m["refined_bits"][k], m["n_corr"])
        rows.append((np.abs(T[:, :3] - R).max(), np.abs(T[:, 3] - t).max(), int((((e2 < tab["max_error"]) != flags) & ~near).sum()),
                     int((e2 < tab["max_error"])[~near].sum()) - int(flags[~near].sum())))
    return rows


@pytest.mark.parametrize("name", REFINE_SCENES)
def test_refine_agrees_with_an_independent_float64_epnp(name):
    rows = refine_census(name)
    assert rows, name
    for dR, dt, flags, counts in rows:
        print("%-12s |R - ref| %.2e  |t - ref| %.2e  flags differing %d" % (name, dR, dt, flags))
        assert flags == 0 and counts == 0, (name, flags, counts)
        assert dR <= REFINE_TOL["R"] and dt <= REFINE_TOL["t"], (name, dR, dt)


@pytest.mark.parametrize("name", ["clean", "outliers", "noisy", "n64", "n65", "n70", "invalid_points", "last_record"])
def test_first_event_reprojects_every_true_inlier_inside_its_gate(name):
    s, m = S.scene(name), S.model(name)
    truth = S.true_inliers(s)
    assert truth.sum() * 2 >= len(truth) and m["n_events"] > 0, name
    k = int(m["events"][0])
    b = int(m["hyp"][k]["best_k"])
    assert m["refined"][b]["ok"]
    flags = M.unpack_bits(m["refined_bits"][b], m["n_corr"])
    assert flags[truth].all(), (name, np.nonzero(truth & ~flags)[0])
    T = m["refined"][b]["Tcw"].reshape(3, 4)
    assert np.abs(T[:, :3] - s["truth"][:3, :3]).max() < 0.02 and np.abs(T[:, 3] - s["truth"][:3, 3]).max() < 0.2, name


def test_select_rows_of_the_model():
    s, m = S.scene("n65"), S.model("n65")
    n_keys, cap = len(s["keys"]), s["capacity"]
    k = int(m["events"][0])
    Tcw, cur, has, status = M.select_rows(m, M.EVENT, k, n_keys, cap, -7, 9)
    b = int(m["hyp"][k]["best_k"])
    assert status == 0 and has.sum() == m["refined"][b]["n_inliers"] and np.array_equal(cur[has == 1], s["f_match"][:n_keys][has == 1]) and (cur[has == 0] == -1).all()
    assert np.array_equal(Tcw.reshape(4, 4)[3], [0, 0, 0, 1])
    Tcw, cur, has, status = M.select_rows(m, M.EXHAUSTED, 0, n_keys, cap, -7, 9)
    assert status == 0 and has.sum() == m["hyp"][m["exhausted"]]["n_inliers"]
    assert M.select_rows(m, M.EVENT, m["n_its"], n_keys, cap, -7, 9)[3] == M.ERR_INVALID
    assert M.select_rows(S.model("below_min"), M.EXHAUSTED, 0, 96, 96, -7, 9)[3] == M.ERR_INVALID
