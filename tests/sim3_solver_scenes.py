"""Scenes of the Sim3Solver port for tests/test_sim3_solver_model.py, tests/test_sim3_solver_host.py (CPU) and
tests/test_sim3_ransac_device.py (GPU).  One KF1 (mpCurrentKF) and candidates built against it: map points in front of both cameras, a
true S12 per candidate, 3-D noise of a centimetre on the inliers and gross 3-D outliers.  A scene is one candidate with everything the
model (tests/sim3_solver_model.py) needs; model(name) computes each scene's rows once and is shared by all tests.

Asserted here, for this file's own seeds: the truncated-gate scene's error really lies in [9.0, 9.21) and the random scenes leave at most
0.1 % of their cases within a relative 1e-3 of a gate (the cap of the float64 comparison)."""
import numpy as np

from tests import sim3_solver_model as M
from tests.sim3_opt_scenes import CAM, KP_DTYPE, NLEVELS, _pose, rot

LDS_SLOTS = 1024                       # ORBFE_SIM3_RANSAC_LDS_SLOTS (include/orbfe.h)
PROB, MIN_INLIERS, MAX_ITS = 0.99, 20, 300      # src/LoopClosing.cc:298, include/Sim3Solver.h:50
ALL_ITS_MIN = 9                        # at 40 correspondences SetRansacParameters keeps all 300 iterations only below 10 minimal inliers (35 at 20)


def sigma2():
    """mvLevelSigma2 as the context's planner forms it (scale factor 1.2f, orbfe_plan.cpp)."""
    sf = float(np.float32(1.2))
    scale = [np.float32(1.0)]
    for _ in range(1, NLEVELS):
        scale.append(np.float32(float(scale[-1]) * sf))
    return np.array([s * s for s in scale], np.float32)


SIGMA2 = sigma2()


def draws(seed, max_its):
    """A draw row: raw rand() values in [0, RAND_MAX]."""
    return np.random.default_rng(seed).integers(0, M.RAND_MAX + 1, (max_its, 3), dtype=np.int64).astype(np.uint32)


def make_kf1(seed, n1, identity=False):
    rng = np.random.default_rng(seed)
    T1w = _pose((0, 0, 0), (0, 0, 0)) if identity else _pose(rng.uniform(-0.3, 0.3, 3), rng.uniform(-2, 2, 3))
    z = rng.uniform(4, 20, n1)
    X1c = np.stack([rng.uniform(-0.45, 0.45, n1) * z, rng.uniform(-0.35, 0.35, n1) * z, z], 1)
    R1, t1 = T1w[:, :3].astype(np.float64), T1w[:, 3].astype(np.float64)
    keys1 = np.zeros(n1, KP_DTYPE)
    keys1["x"], keys1["y"], keys1["octave"] = rng.uniform(20, 620, n1), rng.uniform(20, 460, n1), np.arange(n1) % NLEVELS
    return dict(T1w=T1w, X1c=X1c, pos1=((X1c - t1) @ R1).astype(np.float32), keys1=keys1, valid1=np.ones(n1, np.int32))


def make(kf1, seed, n2=80, n_pairs=40, n_outliers=0, fix_scale=False, noise=0.01, max_its=12, min_inliers=MIN_INLIERS, max_pairs=None, max_kf_n=None,
         invalid=(), identity=False):
    """One candidate against kf1.  invalid: (side, k): pair k's slot on that side gets valid = 0."""
    rng = np.random.default_rng(seed)
    n1 = len(kf1["keys1"])
    T2w = _pose((0, 0, 0), (0, 0, 0)) if identity else _pose(rng.uniform(-0.3, 0.3, 3), rng.uniform(-2, 2, 3))
    s_true = 1.0 if fix_scale else float(rng.uniform(0.8, 1.25))
    R_true, t_true = rot(rng.uniform(-0.08, 0.08, 3)), rng.uniform(-0.5, 0.5, 3)
    keys2 = np.zeros(n2, KP_DTYPE)
    keys2["x"], keys2["y"], keys2["octave"] = rng.uniform(20, 620, n2), rng.uniform(20, 460, n2), (np.arange(n2) * 3 + 1) % NLEVELS
    pos2 = rng.uniform(-5, 5, (n2, 3)).astype(np.float32)
    valid1, valid2 = kf1["valid1"].copy(), (rng.random(n2) < 0.85).astype(np.int32)
    s1 = np.sort(rng.choice(n1, n_pairs, replace=False))
    s2 = rng.choice(n2, n_pairs, replace=False)
    X2c = ((kf1["X1c"][s1] - t_true) @ R_true) / s_true + rng.normal(0, noise, (n_pairs, 3))
    outl = rng.choice(n_pairs, n_outliers, replace=False) if n_outliers else np.zeros(0, np.int64)
    X2c[outl] += rng.uniform(0.3, 1.0, (len(outl), 3)) * rng.choice([-1, 1], (len(outl), 3))
    assert X2c[:, 2].min() > 1.0
    R2, t2 = T2w[:, :3].astype(np.float64), T2w[:, 3].astype(np.float64)
    pos2[s2] = ((X2c - t2) @ R2).astype(np.float32)
    valid2[s2] = 1
    for side, k in invalid:
        (valid1 if side == 1 else valid2)[(s1 if side == 1 else s2)[k]] = 0
    max_pairs = n_pairs if max_pairs is None else max_pairs
    return dict(keys1=kf1["keys1"], pos1=kf1["pos1"], valid1=valid1, T1w=kf1["T1w"], keys2=keys2, pos2=pos2, valid2=valid2, T2w=T2w,
                pairs=np.stack([s1, s2], 1).astype(np.int32), draws=draws(seed + 1000, max_its), fix_scale=int(fix_scale), min_inliers=min_inliers,
                max_its=max_its, max_pairs=max_pairs, max_kf_n=max(n1, n2) if max_kf_n is None else max_kf_n, sigma2=SIGMA2, cam=CAM, prob=PROB,
                its_for_n=M.its_table(max_pairs, PROB, min_inliers, max_its), truth=(R_true, t_true, s_true), outliers=np.sort(outl))


KF1 = make_kf1(1, 96)                 # the batch's common KF1
KF1_WIDE = make_kf1(2, 128)
KF1_BIG = make_kf1(3, LDS_SLOTS + 76)
KF1_ID = make_kf1(4, 96, identity=True)


def _gate_scene():
    """Noise-free, so every hypothesis is the truth up to rounding; then pair J (level 0 in KF1, level 3 in the candidate: gates 9 and
    27) is moved in the candidate until hypothesis K, which does not draw it, sees err1 inside [9.0, 9.21): the reference's size_t gate
    calls that an outlier, a float gate of 9.21 would not."""
    s = make(KF1, 31, noise=0.0)
    J = int(np.nonzero(s["keys1"]["octave"][s["pairs"][:, 0]] == 0)[0][0])
    s["keys2"]["octave"][s["pairs"][J, 1]] = 3
    K = next(k for k in range(s["max_its"]) if J not in M.draw_set(s["draws"][k], len(s["pairs"])))
    base = s["pos2"][s["pairs"][J, 1]].copy()
    lo, hi = 0.0, 0.5
    for _ in range(60):                                        # bisection on the shift; err1 grows with it
        mid = 0.5 * (lo + hi)
        s["pos2"][s["pairs"][J, 1]] = base + np.float32(mid) * s["T2w"][0, :3]
        e1 = _errors(s, K)[0][J]
        if 9.05 <= e1 <= 9.15:
            break
        lo, hi = (mid, hi) if e1 < 9.05 else (lo, mid)
    s["gate_case"] = (K, J)
    return s


def _errors(s, k):
    _, corr, tab = M.filter_pairs(s)
    ids = M.draw_set(s["draws"][k], len(corr))
    _, t, _, sR, sRinv, tinv = M.compute_sim3(tab["X1"][list(ids)].T.copy(), tab["X2"][list(ids)].T.copy(), s["fix_scale"])
    _, e1, e2 = M.check_inliers(tab, sR, t, sRinv, tinv, s["cam"])
    return e1, e2, tab


def _coincident_scene():
    """Identity poses and points of few mantissa bits: pairs 0 1 2 carry one and the same point on either side, and hypothesis 0 is
    made to draw exactly them, so both centred sets are exactly zero: M = 0, N = 0, den == 0."""
    s = make(KF1_ID, 41, identity=True)
    s["pos1"] = s["pos1"].copy()
    for j in range(3):
        s["pos1"][s["pairs"][j, 0]] = (0.5, -0.25, 8.0)
        s["pos2"][s["pairs"][j, 1]] = (1.0, 0.5, 4.0)
    N = len(s["pairs"])
    # raw values whose RandomInt lands on 0, 1, 2 at d = N, N - 1, N - 2 (position 0 holds N - 1 after the first draw)
    s["draws"][0] = [0, int(np.ceil(1 * 2147483648.0 / (N - 1))), int(np.ceil(2 * 2147483648.0 / (N - 2)))]
    assert M.draw_set(s["draws"][0], N) == (0, 1, 2)
    return s


SPECS = {
    "clean": lambda: make(KF1, 11, max_its=MAX_ITS, min_inliers=ALL_ITS_MIN),
    "outliers": lambda: make(KF1, 12, n_outliers=10, max_its=MAX_ITS, min_inliers=ALL_ITS_MIN),
    "random_b": lambda: make(KF1, 13, n_outliers=10, max_its=MAX_ITS, min_inliers=ALL_ITS_MIN),
    "random_c": lambda: make(KF1, 14, n_outliers=10, max_its=MAX_ITS, min_inliers=ALL_ITS_MIN, noise=0.02),
    "fix_scale": lambda: make(KF1, 15, n_outliers=6, fix_scale=True),
    "n64": lambda: make(KF1_WIDE, 16, n2=128, n_pairs=64, n_outliers=12),
    "n65": lambda: make(KF1_WIDE, 17, n2=128, n_pairs=65, n_outliers=12),
    "n70": lambda: make(KF1_WIDE, 18, n2=128, n_pairs=70, n_outliers=12),
    "hbm": lambda: make(KF1_BIG, 19, n2=LDS_SLOTS + 40, n_pairs=LDS_SLOTS + 1, n_outliers=200),
    "invalid_slots": lambda: make(KF1, 20, n_outliers=6, invalid=((1, 3), (2, 7), (1, 20), (2, 20))),
    "below_min": lambda: make(KF1, 21, n_pairs=15),
    "at_min": lambda: make(KF1, 22, n_pairs=20),
    "gate": _gate_scene,
    "coincident": _coincident_scene,
    "cand_a": lambda: make(KF1, 23, n_outliers=8, n2=80, max_kf_n=96),
    "cand_b": lambda: make(KF1, 24, n_outliers=5, n2=72, n_pairs=33, max_pairs=40, max_kf_n=96),
}
RANDOM_SCENES = ["outliers", "random_b", "random_c"]       # 40 correspondences, 30 inliers, 300 hypotheses
DEVICE_SCENES = [n for n in SPECS if n not in ("random_b", "random_c", "cand_a", "cand_b")]
_scenes, _models = {}, {}


def scene(name):
    if name not in _scenes:
        _scenes[name] = SPECS[name]()
    return _scenes[name]


def model(name):
    if name not in _models:
        _models[name] = M.run(scene(name))
    return _models[name]


def gate_case():
    """(K, J, err1, err2, gate1, gate2) of the truncated-gate scene, asserted to lie where the scene wants it."""
    s = scene("gate")
    K, J = s["gate_case"]
    e1, e2, tab = _errors(s, K)
    assert tab["g1"][J] == 9.0 and tab["g2"][J] == 27.0
    assert 9.0 <= e1[J] < np.float32(9.21) and e2[J] < tab["g2"][J], (e1[J], e2[J])
    return K, J, float(e1[J]), float(e2[J]), float(tab["g1"][J]), float(tab["g2"][J])


def near_gate_census(name):
    """Over every (hypothesis, correspondence) of a random scene: (cases, left out, disagreements outside them, max |R, t, s - float64|).
    A case is left out when its float64 error lies within a relative 1e-3 of its gate."""
    s, m = scene(name), model(name)
    tab, N = m["table"], m["n_corr"]
    cases = left = bad = 0
    dev = 0.0
    for k in range(m["n_its"]):
        e1, e2, R, t, sc = M.reference_errors(tab, m["sets"][k], s["fix_scale"], s["cam"])
        flags = np.array([(m["bits"][k][j >> 5] >> np.uint32(j & 31)) & 1 for j in range(N)], bool)
        near = (np.abs(e1 - tab["g1"]) <= 1e-3 * tab["g1"]) | (np.abs(e2 - tab["g2"]) <= 1e-3 * tab["g2"])
        ref = (e1 < tab["g1"]) & (e2 < tab["g2"])
        cases += N
        left += int(near.sum())
        bad += int(((ref != flags) & ~near).sum())
        h = m["hyp"][k]
        dev = max(dev, np.abs(h["R12"].reshape(3, 3) - R).max(), np.abs(h["t12"] - t).max(), abs(float(h["s12"]) - sc))
    assert left * 1000 <= cases, (name, left, cases)               # the cap of the comparison, for this file's own seeds
    return cases, left, bad, dev
