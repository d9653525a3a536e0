"""Scenes of the PnPsolver port for tests/test_pnp_solver_model.py, tests/test_pnp_solver_host.py (CPU) and
tests/test_pnp_ransac_device.py (GPU).  A frame (undistorted keypoints, a true pose) and candidates built against it: a keyframe's map
points, a row of SearchByBoW matches, the projections of the matched points with pixel noise, and gross outliers (keypoints somewhere
else in the image).  A scene is one candidate with everything the model (tests/pnp_solver_model.py) needs; model(name) computes each
scene's rows once and is shared by all tests.  The parameters are Tracking::Relocalization's (src/Tracking.cc:1488): probability 0.99,
10 inliers, 300 iterations, a minimal set of 4, epsilon 0.5, th2 5.991, iterate(5) -- where a scene says nothing else.

Asserted here, for this file's own seeds and draws: the scenes built for a property (a lone record on the last iteration, more than four
records, a NaN hypothesis) have it."""
import numpy as np

from tests import pnp_solver_model as M
from tests.sim3_opt_scenes import CAM, KP_DTYPE, NLEVELS, rot
from tests.sim3_solver_scenes import SIGMA2

LDS_SLOTS = 1024                       # ORBFE_PNP_RANSAC_LDS_SLOTS (include/orbfe.h)
PROB, MIN_INLIERS, MAX_ITS, EPSILON, TH2, ITERATE = 0.99, 10, 300, 0.5, 5.991, 5


def draws(seed, max_its):
    """A draw row: raw rand() values in [0, RAND_MAX]."""
    return np.random.default_rng(seed).integers(0, M.RAND_MAX + 1, (max_its, 4), dtype=np.int64).astype(np.uint32)


def raw_for(ids, N):
    """Raw values whose RandomInt and swap-with-back-and-pop give exactly `ids`."""
    avail, raw = list(range(N)), []
    for want in ids:
        p = avail.index(want)
        r = int(np.ceil(p * 2147483648.0 / len(avail)))
        assert M.random_int(r, len(avail)) == p
        raw.append(r)
        avail[p] = avail[-1]
        avail.pop()
    assert M.draw_set(raw, N) == list(ids)
    return raw


def make_frame(seed, n_keys):
    """The true pose and the keypoints' octaves; pixel positions are set per candidate (a frame shared by candidates keeps the positions
    of the first that sets them: candidates of one batch use disjoint keypoints)."""
    rng = np.random.default_rng(seed)
    keys = np.zeros(n_keys, KP_DTYPE)
    keys["x"], keys["y"], keys["octave"] = rng.uniform(20, 620, n_keys), rng.uniform(20, 460, n_keys), np.arange(n_keys) % NLEVELS
    keys["size"], keys["class_id"] = 31.0, -1
    return dict(keys=keys, R=rot(rng.uniform(-0.3, 0.3, 3)), t=rng.uniform(-1.5, 1.5, 3), taken=np.zeros(n_keys, bool))


def make(frame, seed, n_kf=80, n_match=40, n_outliers=0, noise=0.5, max_its=12, min_inliers=MIN_INLIERS, epsilon=EPSILON, n_iterations=ITERATE,
         capacity=None, invalid=(), depth=(4.0, 20.0), max_kf_n=None):
    """One candidate keyframe against `frame`.  invalid: matched pairs (by rank) whose map point gets valid = 0."""
    rng = np.random.default_rng(seed)
    keys = frame["keys"]
    n_keys = len(keys)
    free = np.nonzero(~frame["taken"])[0]
    kp = np.sort(rng.choice(free, n_match, replace=False))
    frame["taken"][kp] = True
    slots = rng.choice(n_kf, n_match, replace=False)
    z = rng.uniform(depth[0], depth[1], n_match)
    Xc = np.stack([rng.uniform(-0.5, 0.5, n_match) * z, rng.uniform(-0.38, 0.38, n_match) * z, z], 1)
    pos = rng.uniform(-5, 5, (n_kf, 3)).astype(np.float32)
    pos[slots] = ((Xc - frame["t"]) @ frame["R"]).astype(np.float32)          # Xw = R^T (Xc - t)
    Xc = pos[slots].astype(np.float64) @ frame["R"].T + frame["t"]
    uv = np.stack([CAM[0] * Xc[:, 0] / Xc[:, 2] + CAM[2], CAM[1] * Xc[:, 1] / Xc[:, 2] + CAM[3]], 1) + rng.normal(0, noise, (n_match, 2)) * (noise > 0)
    outl = np.sort(rng.choice(n_match, n_outliers, replace=False)) if n_outliers else np.zeros(0, np.int64)
    uv[outl] = np.stack([rng.uniform(20, 620, len(outl)), rng.uniform(20, 460, len(outl))], 1)
    keys["x"][kp], keys["y"][kp] = uv[:, 0], uv[:, 1]
    f_match = np.full(n_keys, -1, np.int32)
    f_match[kp] = slots
    valid = (rng.random(n_kf) < 0.85).astype(np.int32)
    valid[slots] = 1
    for k in invalid:
        valid[slots[k]] = 0
    capacity = n_keys if capacity is None else capacity
    Tcw = np.eye(4)
    Tcw[:3, :3], Tcw[:3, 3] = frame["R"], frame["t"]
    return dict(keys=keys, f_match=f_match, pos=pos, valid=valid, draws=draws(seed + 1000, max_its), capacity=capacity, max_its=max_its,
                min_inliers=min_inliers, epsilon=epsilon, n_iterations=n_iterations, th2=TH2, prob=PROB, sigma2=SIGMA2, cam=CAM,
                max_kf_n=n_kf if max_kf_n is None else max_kf_n, its_for_n=M.its_table(capacity, PROB, min_inliers, MAX_ITS, epsilon),
                truth=Tcw, kp=kp, slots=slots, outliers=outl, frame=frame)


def true_inliers(s):
    """Per correspondence of the scene (the model's order): not an outlier by construction."""
    order = np.argsort(s["kp"])
    flags = np.ones(len(s["kp"]), bool)
    flags[s["outliers"]] = False
    keep = s["valid"][s["slots"]] != 0
    return flags[order][keep[order]]


def _with_draws(s, k, ids):
    N = M.filter_frame(s)[1].shape[0]
    s["draws"][k] = raw_for(ids, N)
    return s


def _degenerate_scene():
    """Hypothesis 0 draws four correspondences that carry one and the same map point position (PW0tPW0 = 0, every control point on the
    centroid, CC = 0: its pseudo-inverse is 0, rho = 0, the betas divide 0 by 0); hypothesis 1 draws four coplanar points (z = 8 in the
    world: one zero singular value of PW0tPW0, a singular CC)."""
    s = make(make_frame(41, 96), 41, noise=0.0)
    order = np.argsort(s["kp"])
    sl = s["slots"][order]
    for j in range(4):
        s["pos"][sl[j]] = (0.5, -0.25, 8.0)
    for j, xy in zip(range(4, 8), ((1.0, 0.5), (-1.5, 0.25), (0.75, -1.0), (-0.5, -0.75))):
        s["pos"][sl[j]] = (xy[0], xy[1], 8.0)
    _with_draws(s, 0, [0, 1, 2, 3])
    return _with_draws(s, 1, [4, 5, 6, 7])


def _last_record_scene():
    """Twelve iterations; the first eleven draw at least two gross outliers each and stay below mRansacMinInliers, the last draws four
    inliers: the only record, and its refinement succeeds, so the only event is the last iteration."""
    s = make(make_frame(43, 96), 43, n_outliers=14, noise=0.3)
    N = M.filter_frame(s)[1].shape[0]
    inl = true_inliers(s)
    bad, good = np.nonzero(~inl)[0], np.nonzero(inl)[0]
    rng = np.random.default_rng(7)
    for k in range(11):
        ids = list(rng.choice(bad, 2, replace=False)) + list(rng.choice(good, 2, replace=False))
        s["draws"][k] = raw_for([int(i) for i in ids], N)
    s["draws"][11] = raw_for([int(i) for i in good[[0, 7, 13, 21]]], N)
    return s


def _hbm_scene():
    """One correspondence more than the LDS holds; the four iterations draw true inliers, so the refinement runs on the table in HBM too."""
    s = make(make_frame(19, LDS_SLOTS + 76), 19, n_kf=LDS_SLOTS + 40, n_match=LDS_SLOTS + 1, n_outliers=300, max_its=4)
    good = np.nonzero(true_inliers(s))[0]
    for k, pick in enumerate(([0, 100, 300, 600], [5, 205, 405, 705], [11, 111, 311, 511], [2, 222, 444, 666])):
        _with_draws(s, k, [int(i) for i in good[pick]])
    return s


SPECS = {
    "clean": lambda: make(make_frame(11, 96), 11, max_its=MAX_ITS, n_iterations=MAX_ITS),
    "outliers": lambda: make(make_frame(12, 96), 12, n_outliers=20, max_its=MAX_ITS, n_iterations=MAX_ITS, epsilon=0.3),
    "noisy": lambda: make(make_frame(13, 96), 13, n_outliers=10, noise=1.0, max_its=60, n_iterations=60, epsilon=0.3),
    "n64": lambda: make(make_frame(16, 128), 16, n_kf=128, n_match=64, n_outliers=12),
    "n65": lambda: make(make_frame(17, 128), 17, n_kf=128, n_match=65, n_outliers=12),
    "n70": lambda: make(make_frame(28, 128), 28, n_kf=128, n_match=70, n_outliers=12),
    "hbm": lambda: _hbm_scene(),
    "invalid_points": lambda: make(make_frame(20, 96), 20, n_outliers=6, invalid=(3, 7, 20)),
    "n4": lambda: make(make_frame(21, 96), 21, n_match=4, min_inliers=4, noise=0.0),
    "below_min": lambda: make(make_frame(22, 96), 22, n_match=8),
    "at_min": lambda: make(make_frame(23, 96), 23, n_match=10, noise=0.0),
    "degenerate": _degenerate_scene,
    "last_record": _last_record_scene,
    "many_records": lambda: make(make_frame(61, 96), 61, n_outliers=4, noise=3.0, min_inliers=4, epsilon=0.1, max_its=40, n_iterations=40),
}
DEVICE_SCENES = list(SPECS)
_scenes, _models, _stages = {}, {}, {}
_BATCH = {}


def batch_scenes():
    """Three candidates against ONE frame (disjoint keypoints), as one batch call takes them: the same parameters, one table."""
    if not _BATCH:
        f = make_frame(50, 128)
        _BATCH["s"] = [make(f, 51, n_outliers=8, max_kf_n=96), make(f, 52, n_kf=72, n_match=33, n_outliers=5, max_kf_n=96), make(f, 53, n_match=30, max_kf_n=96)]
        for s in _BATCH["s"]:
            s["keys"] = f["keys"]                                # the frame as all three left it
    return _BATCH["s"]


def scene(name):
    if name not in _scenes:
        _scenes[name] = SPECS[name]()
    return _scenes[name]


def model(name):
    if name not in _models:
        _stages[name] = {}
        _models[name] = M.run(scene(name), _stages[name])
    return _models[name]


def stages(name):
    model(name)
    return _stages[name]


def records(m):
    """The record holders of a model's rows."""
    return sorted(set(int(b) for b in m["hyp"]["best_k"][:m["n_its"]] if b >= 0))
