"""Scenes of orbfe_enqueue_optimize_sim3 for tests/test_sim3_opt_model.py (CPU) and tests/test_sim3_opt_device.py (GPU): two keyframes,
map points in front of both cameras, observations with Gaussian pixel noise scaled by the level sigma, octaves over all 8 levels, and an
initial S12 off the truth by a few degrees, a few percent of the baseline and, where the scale is free, about 10 % in scale.

Condition on every scene (test_sim3_opt_model.test_every_scene_keeps_its_distance_from_th2): no correspondence has a chi2 within 1 % of
th2 at either classification of the float64 model, so the device's flags may be compared without leaving out an entry.  The seeds below
were chosen so that the model alone meets it.  model(name) computes each scene's reference once and is shared by all tests.
"""
import numpy as np

from tests import sim3_opt_model as M

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
CAM = (500.0, 500.0, 320.0, 240.0)   # tests/test_matchers.py: FX, FY, CX, CY, the camera of tests.device_arrays.context()
NLEVELS = 8
TH2 = 10.0                           # src/LoopClosing.cc:362
LDS_SLOTS = 2048                     # ORBFE_SIM3_OPT_LDS_SLOTS (include/orbfe.h)


def inv_sigma2():
    """mvInvLevelSigma2 as the context's planner forms it (scale factor 1.2f, orbfe_plan.cpp)."""
    sf = float(np.float32(1.2))
    scale = [np.float32(1.0)]
    for _ in range(1, NLEVELS):
        scale.append(np.float32(float(scale[-1]) * sf))
    return np.array([np.float32(1.0) / (s * s) for s in scale], np.float32)


INV_SIGMA2 = inv_sigma2()


def rot(rv):
    rv = np.asarray(rv, np.float64)
    th = np.linalg.norm(rv)
    if th == 0:
        return np.eye(3)
    k = rv / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def _pose(rv, t):
    T = np.zeros((3, 4), np.float32)
    T[:, :3] = rot(rv)
    T[:, 3] = t
    return T


def make(seed, n1=96, n2=80, n_corr=40, n_outliers=0, fix_scale=False, noise=0.5, split_prior=False, invalid=(), bad_match=None, bad_octave=None,
         off=(3.0, 0.04, 0.10)):
    """One scene.  off = (degrees, fraction of the baseline, relative scale) of the initial S12 from the truth.  invalid: pairs
    (side, k): correspondence k gets valid = 0 on side 1 or 2.  bad_match = (k, value): correspondence k's match12 entry becomes `value`;
    bad_octave = (side, k, value): the keypoint of correspondence k on that side gets that octave."""
    rng = np.random.default_rng(seed)
    T1w = _pose(rng.uniform(-0.3, 0.3, 3), rng.uniform(-2, 2, 3))
    T2w = _pose(rng.uniform(-0.3, 0.3, 3), rng.uniform(-2, 2, 3))
    s_true = 1.0 if fix_scale else float(rng.uniform(0.8, 1.25))
    R_true, t_true = rot(rng.uniform(-0.08, 0.08, 3)), rng.uniform(-0.5, 0.5, 3)      # camera 2 -> camera 1; baseline = |t|
    fx, fy, cx, cy = CAM
    keys1, keys2 = np.zeros(n1, KP_DTYPE), np.zeros(n2, KP_DTYPE)
    for k, n in ((keys1, n1), (keys2, n2)):                                          # every slot holds a plausible keypoint and point
        k["x"], k["y"], k["octave"] = rng.uniform(20, 620, n), rng.uniform(20, 460, n), rng.integers(0, NLEVELS, n)
    pos1, pos2 = rng.uniform(-5, 5, (n1, 3)).astype(np.float32), rng.uniform(-5, 5, (n2, 3)).astype(np.float32)
    valid1, valid2 = (rng.random(n1) < 0.85).astype(np.int32), (rng.random(n2) < 0.85).astype(np.int32)
    s1 = np.sort(rng.choice(n1, n_corr, replace=False)) if n_corr else np.zeros(0, np.int64)
    s2 = rng.choice(n2, n_corr, replace=False) if n_corr else np.zeros(0, np.int64)
    z = rng.uniform(4, 20, n_corr)
    X1c = np.stack([rng.uniform(-0.45, 0.45, n_corr) * z, rng.uniform(-0.35, 0.35, n_corr) * z, z], 1)
    X2c = ((X1c - t_true) @ R_true) / s_true                                         # S12^-1
    assert n_corr == 0 or X2c[:, 2].min() > 1.0
    R1, t1, R2, t2 = T1w[:, :3].astype(np.float64), T1w[:, 3].astype(np.float64), T2w[:, :3].astype(np.float64), T2w[:, 3].astype(np.float64)
    pos1[s1] = ((X1c - t1) @ R1).astype(np.float32)
    pos2[s2] = ((X2c - t2) @ R2).astype(np.float32)
    lv1, lv2 = np.arange(n_corr) % NLEVELS, (np.arange(n_corr) * 3 + 1) % NLEVELS    # all 8 levels on both sides
    sig = np.float64(1.2) ** np.arange(NLEVELS)
    e1, e2 = rng.normal(0, noise, (n_corr, 2)) * sig[lv1][:, None], rng.normal(0, noise, (n_corr, 2)) * sig[lv2][:, None]
    outl = rng.choice(n_corr, n_outliers, replace=False) if n_outliers else np.zeros(0, np.int64)
    for j, k in enumerate(outl):                                                     # gross outliers of 20 to 40 px, either image
        ang, mag = rng.uniform(0, 2 * np.pi), rng.uniform(20, 40)
        (e1 if j % 2 == 0 else e2)[k] += mag * np.array([np.cos(ang), np.sin(ang)])
    keys1["x"][s1], keys1["y"][s1], keys1["octave"][s1] = fx * X1c[:, 0] / X1c[:, 2] + cx + e1[:, 0], fy * X1c[:, 1] / X1c[:, 2] + cy + e1[:, 1], lv1
    keys2["x"][s2], keys2["y"][s2], keys2["octave"][s2] = fx * X2c[:, 0] / X2c[:, 2] + cx + e2[:, 0], fy * X2c[:, 1] / X2c[:, 2] + cy + e2[:, 1], lv2
    valid1[s1], valid2[s2] = 1, 1
    match12 = np.full(n1, -1, np.int32)
    match12[s1] = s2
    prior12 = None
    if split_prior:                                                                  # the RANSAC inliers' share, disjoint from SearchBySim3's
        prior12 = np.full(n1, -1, np.int32)
        mine = s1[::3]
        prior12[mine] = match12[mine]
        match12[mine] = -1
        prior12[[i for i in range(n1) if match12[i] < 0 and prior12[i] < 0][:2]] = -5   # any negative prior entry means "none"
    for side, k in invalid:
        (valid1 if side == 1 else valid2)[(s1 if side == 1 else s2)[k]] = 0
    if bad_match is not None:
        match12[s1[bad_match[0]]] = bad_match[1]
    if bad_octave is not None:
        side, k, val = bad_octave
        (keys1 if side == 1 else keys2)["octave"][(s1 if side == 1 else s2)[k]] = val
    deg, frac, rel = off
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    dv = rng.normal(size=3); dv /= np.linalg.norm(dv)
    R12 = (rot(np.radians(deg) * ax) @ R_true).astype(np.float32)
    t12 = (t_true + frac * np.linalg.norm(t_true) * dv).astype(np.float32)
    s12 = np.float32(s_true if fix_scale else s_true * (1 + rel))
    return dict(keys1=keys1, keys2=keys2, pos1=pos1, pos2=pos2, valid1=valid1, valid2=valid2, T1w=T1w, T2w=T2w, s12=s12, R12=R12, t12=t12,
                th2=TH2, fix_scale=int(fix_scale), match12=match12, prior12=prior12, truth=(R_true, t_true, s_true), slots1=s1, slots2=s2,
                outliers=np.sort(outl), params=None)


SPECS = {
    "clean": dict(seed=11),
    "outliers": dict(seed=12, n_outliers=6),
    "fix_scale": dict(seed=13, fix_scale=True, n_outliers=3),
    "early": dict(seed=14, n_corr=12, n_outliers=4),
    "none": dict(seed=15, n_corr=0),
    "kf1_empty": dict(seed=16, n1=0, n_corr=0),
    "prior": dict(seed=17, n_outliers=4, split_prior=True),
    "invalid_slots": dict(seed=18, n_outliers=2, invalid=((1, 3), (2, 7), (1, 20), (2, 20))),
    "bad_match_high": dict(seed=19, bad_match=(5, 80)),          # == kf2's n
    "bad_match_low": dict(seed=19, bad_match=(5, -2)),
    "bad_octave1": dict(seed=20, bad_octave=(1, 9, NLEVELS)),
    "bad_octave2": dict(seed=20, bad_octave=(2, 9, -1)),
    "scratch_table": dict(seed=21, n1=LDS_SLOTS + 257, n2=300, n_corr=64, n_outliers=5),   # more slots than the LDS table holds
    "noiseless": dict(seed=22, noise=0.0),
    "corr60": dict(seed=23, n1=1500, n2=1400, n_corr=60, n_outliers=6),                     # the two latency shapes of DESIGN.md
    "corr300": dict(seed=24, n1=1500, n2=1400, n_corr=300, n_outliers=30),
}
DEVICE_SCENES = ["clean", "outliers", "fix_scale", "early", "none", "kf1_empty", "prior", "invalid_slots", "bad_match_high", "bad_match_low",
                 "bad_octave1", "bad_octave2", "scratch_table"]
_SCENES, _MODELS = {}, {}


def scene(name):
    if name not in _SCENES:
        _SCENES[name] = make(**SPECS[name])
    return _SCENES[name]


def run_model(s, **over):
    a = dict(s, **over)
    return M.optimize_sim3(a["keys1"], a["T1w"], a["pos1"], a["valid1"], a["keys2"], a["T2w"], a["pos2"], a["valid2"], a["s12"], a["R12"], a["t12"],
                           a["th2"], a["fix_scale"], a["match12"], CAM, INV_SIGMA2, NLEVELS, prior12=a["prior12"], params=a["params"])


def model(name):
    """The model's result on scene(name), computed once and never changed."""
    if name not in _MODELS:
        _MODELS[name] = run_model(scene(name))
    return _MODELS[name]


def margin(res, th2=TH2):
    """Smallest |chi2 / th2 - 1| over the chi2 values the two classifications compare with th2 (inf when none)."""
    vals = []
    if res["chi_first"] is not None:
        vals.append(res["chi_first"].reshape(-1))
    if res["chi_second"] is not None:
        vals.append(res["chi_second"][res["active_second"]].reshape(-1))
    vals = np.concatenate(vals) if vals else np.zeros(0)
    return float(np.abs(vals / th2 - 1).min()) if vals.size else float("inf")


# ================================================================ cases of the single blocks (tests/test_sim3_opt_model.py proves the
# model on them, tests/test_sim3_blocks.py compares the device blocks with the model on the same lists)
def rts_cases():
    """(name, R, t, s, branch of Quaterniond(R)): the trace branch, the three others, and a matrix that is not orthonormal."""
    O = np.array([[0, -3e-6, 2e-6], [3e-6, 0, -1e-6], [-2e-6, 1e-6, 0]])
    return [("trace", rot((0.3, -0.2, 0.1)), (0.1, -0.2, 0.3), 1.1, "trace"),
            ("i0", rot((3.1, 0.05, -0.02)), (0.5, 0.0, -0.25), 0.9, 0),
            ("i1", rot((0.04, 3.12, 0.03)), (-0.4, 0.3, 0.2), 1.0, 1),
            ("i2", rot((-0.03, 0.02, 3.13)), (0.0, 0.7, -0.6), 2.5, 2),
            ("identity", np.eye(3), (0.0, 0.0, 0.0), 1.0, "trace"),
            ("not_orthonormal", np.eye(3) + O + O @ O, (1.0, 2.0, 3.0), 0.5, "trace")]


def exp_cases():
    """(name, u[7], (|sigma| < eps, theta < eps), kind).  kind 'expm': inside its branch's range of validity the closed form equals the
    matrix exponential of the similarity generator to 1e-12 (theta <= 1e-7 where R = I + Omega + Omega^2 is used: the missing half of
    Omega^2 is 5e-15; sigma <= 1e-14 where C = 1 is used); kind 'model': next to the 1e-5 thresholds the branch is g2o's approximation,
    not expm, and the device is compared with the model only."""
    rng = np.random.default_rng(31)
    ax = np.array([0.6, -0.64, 0.48])
    ups = np.array([0.5, -0.25, 0.125])
    cs = []
    for k in range(6):
        cs.append(("big_big%d" % k, np.concatenate([rng.uniform(-1.5, 1.5, 3), rng.uniform(-2, 2, 3), [rng.uniform(-0.4, 0.4)]]), (False, False), "expm"))
    for k, sg in enumerate([0.0, 1e-14, -1e-14]):
        cs.append(("smallsigma_big%d" % k, np.concatenate([rng.uniform(-1.5, 1.5, 3), rng.uniform(-2, 2, 3), [sg]]), (True, False), "expm"))
    for k, (th, sg) in enumerate([(1e-7, 0.3), (0.0, -0.25), (1e-8, 0.1)]):
        cs.append(("big_smalltheta%d" % k, np.concatenate([th * ax, ups, [sg]]), (False, True), "expm"))
    for k, (th, sg) in enumerate([(1e-7, 0.0), (0.0, 0.0), (1e-8, 1e-14)]):
        cs.append(("small_small%d" % k, np.concatenate([th * ax, ups, [sg]]), (True, True), "expm"))
    for d in range(7):                                           # the updates of the numeric Jacobian itself
        for sgn in (1.0, -1.0):
            u = np.zeros(7); u[d] = sgn * 1e-9
            cs.append(("jac_%d%s" % (d, "+" if sgn > 0 else "-"), u, (True, True), "expm"))
    cs.append(("theta_below", np.concatenate([0.99999e-5 * ax, ups, [0.2]]), (False, True), "model"))
    cs.append(("theta_above", np.concatenate([1.00001e-5 * ax, ups, [0.2]]), (False, False), "model"))
    cs.append(("sigma_below", np.concatenate([0.7 * ax, ups, [0.99999e-5]]), (True, False), "model"))
    cs.append(("sigma_above", np.concatenate([0.7 * ax, ups, [-1.00001e-5]]), (False, False), "model"))
    cs.append(("both_below", np.concatenate([0.99999e-5 * ax, ups, [0.99999e-5]]), (True, True), "model"))
    for a in range(3):                                           # a rotation next to pi: Quaterniond(R) leaves the trace branch
        w = np.array([0.004, -0.003, 0.002]); w[a] = np.pi - 5e-4
        cs.append(("near_pi_axis%d" % a, np.concatenate([w, [0.3, -0.7, 0.2, 0.15]]), (False, False), "expm"))
    return cs


def sim3_cases():
    """Random Sim3s as g2o holds them after a few products: quaternions a little off unit norm.  (name, A[8], B[8], point[3])."""
    rng = np.random.default_rng(32)
    cs = []
    for k in range(12):
        def one():
            q = M.quat_of_matrix(rot(rng.uniform(-2.5, 2.5, 3)))
            return np.concatenate([np.array(q) * (1 + rng.uniform(-1e-3, 1e-3)), rng.uniform(-3, 3, 3), [rng.uniform(0.5, 2.0)]])
        cs.append(("rand%d" % k, one(), one(), rng.uniform(-5, 5, 3)))
    return cs


def pivot_matrix7(K, Cc, seed):
    """tests/pose_blocks_model.pivot_matrix for 7 x 7: symmetric, strictly diagonally dominant, the diagonal ordered so that steps
    0 .. K-1 keep their place and step K exchanges with Cc."""
    rng = np.random.default_rng(seed)
    d = np.empty(7)
    rest = 200.0
    for i in range(7):
        if i < K:
            d[i] = 700.0 - 40.0 * i
        elif i == Cc:
            d[i] = 300.0
        else:
            d[i] = rest
            rest -= 25.0
    H = rng.uniform(-8, 8, (7, 7))
    H = (H + H.T) / 2
    H[np.diag_indices(7)] = d + rng.uniform(0, 1, 7)
    return H, rng.uniform(-50, 50, 7)


def ldlt7_cases():
    """(name, H 7x7, b, lambda): every one of the 21 pivot exchanges, no exchange, an exchange at every step, an indefinite matrix (x
    stays untouched), a zero row and column, the fix_scale system (row and column 6 zero, lambda alone on its diagonal), large lambdas."""
    cs = []
    for K in range(6):
        for Cc in range(K + 1, 7):
            H, b = pivot_matrix7(K, Cc, 200 + 10 * K + Cc)
            cs.append(("swap_%d_%d" % (K, Cc), H, b, 0.0))
    H, b = pivot_matrix7(0, 0, 7)
    H[np.diag_indices(7)] = [700, 600, 500, 400, 300, 200, 100]
    cs.append(("no_exchange", H.copy(), b, 0.0))
    H[np.diag_indices(7)] = [100, 700, 600, 500, 400, 300, 200]
    cs.append(("exchange_every_step", H.copy(), b, 0.0))
    cs.append(("indefinite", np.diag([4.0, 1.0, -2.0, 3.0, 5.0, 6.0, 7.0]), np.ones(7), 0.0))
    Hz, bz = pivot_matrix7(1, 4, 8)
    Hz[2, :] = 0.0; Hz[:, 2] = 0.0
    cs.append(("zero_row_col", Hz, bz, 0.0))
    Hf, bf = pivot_matrix7(0, 3, 9)
    Hf[6, :] = 0.0; Hf[:, 6] = 0.0; bf[6] = 0.0
    cs.append(("fix_scale", Hf, bf, 0.25))
    rng = np.random.default_rng(33)
    for lam in (1e-3, 1.0, 1e6, 1e12):
        Mx = rng.normal(size=(7, 7)) * rng.uniform(0.1, 100, 7)
        cs.append(("lambda_%g" % lam, Mx @ Mx.T + 1e-3 * np.eye(7), rng.normal(size=7), lam))
    return cs


def eval_cases():
    """(name, Table, estimate, fix_scale): correspondence tables of 1 to 300 rows at the scene's INITIAL estimate (a few degrees off: many
    edges above the Huber threshold, many below), a tenth of the rows removed; and one at the model's optimum (all below)."""
    cs = []
    for k, n in enumerate([1, 15, 16, 17, 255, 256, 257, 300]):
        s = make(seed=40 + k, n1=n + 30, n2=n + 20, n_corr=n, n_outliers=n // 8, fix_scale=(k % 2 == 1))
        T, _, _ = M.build_table(s["keys1"], s["T1w"], s["pos1"], s["valid1"], s["keys2"], s["T2w"], s["pos2"], s["valid2"], None, s["match12"], INV_SIGMA2, NLEVELS)
        if n > 1:
            T.active[np.random.default_rng(50 + k).random(n) < 0.1] = False
        est = M.sim3(s["R12"].astype(np.float64), s["t12"].astype(np.float64), float(s["s12"]))
        cs.append(("n%d" % n, T, est, bool(s["fix_scale"])))
    r = model("outliers")
    cs.append(("optimum", r["table"], M.unpack(r["S12"]), False))
    return cs


_EVAL = {}


def eval_refs():
    """eval_cases() and the model's pass on each: (cases, [(H, b, chi2, count, mag_H, mag_b, mag_chi)]), computed once.  mag_H and mag_b
    are what the numeric Jacobian's noise is relative to: max over entries of sum_k |J|^T w |J| and of sum_k |J|^T w |e|."""
    if not _EVAL:
        cs, refs = eval_cases(), []
        delta = float(np.float32(np.sqrt(np.float32(TH2))))
        for name, T, est, fix in cs:
            H, b, chi, cnt, J12, J21 = M.evaluate(T, est, fix, CAM, delta)
            magH, magb, magc = np.zeros((7, 7)), np.zeros(7), 0.0
            for (J, P, obs, info, S) in ((J12, T.P2, T.obs1, T.info1, est), (J21, T.P1, T.obs2, T.info2, M.sim3_inverse(est))):
                e0, e1 = M.edge_error(S, CAM, P, obs)
                for k in range(len(T)):
                    if not T.active[k]:
                        continue
                    chi_k = info[k] * (e0[k] ** 2 + e1[k] ** 2)
                    w = info[k] * M.huber(chi_k, delta)[1]
                    magH += w * (np.outer(np.abs(J[k, 0]), np.abs(J[k, 0])) + np.outer(np.abs(J[k, 1]), np.abs(J[k, 1])))
                    magb += w * (np.abs(J[k, 0]) * abs(e0[k]) + np.abs(J[k, 1]) * abs(e1[k]))
                    magc += 2 * info[k] * (abs(e0[k]) * (2 * abs(obs[k, 0]) + abs(e0[k])) + abs(e1[k]) * (2 * abs(obs[k, 1]) + abs(e1[k])))
            refs.append((H, b, chi, cnt, float(magH.max()), float(magb.max()), magc))
        _EVAL["v"] = (cs, refs)
    return _EVAL["v"]
