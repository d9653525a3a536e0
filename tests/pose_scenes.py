"""Seeded PoseOptimization scenes of 12 to 300 slots that, between them, take every branch of the solver that honest input
reaches (tests/test_pose_census.py).  test_pose.scene() fixes the camera, the depth range and the lateral spread, so the order of
H's diagonal never changes there and 3 of the 15 pivot exchanges ever run, from one quaternion branch.  Here the camera, the depth
range, the lateral spread and offset, the stereo fraction and the rotation vary.

The scenes were chosen on the CPU with the oracle alone (its trace, oracle.pose_trace()): each keeps a classification margin of
at least 1e-4, is insensitive to the order of its edges and has |t| < 1 m -- test_pose_census.py asserts all three, so that the
GPU comparison at test_pose.POSE_ATOL means what it means in test_pose.py.
"""
import numpy as np

from oracle import oracle as O

CAMS = [dict(fx=718.856, fy=718.856, cx=607.1928, cy=185.2157, bf=386.1448),
        dict(fx=300.0, fy=900.0, cx=320.0, cy=240.0, bf=40.0),
        dict(fx=900.0, fy=300.0, cx=320.0, cy=240.0, bf=0.0)]
INV_SIGMA2 = (1.0 / (np.float32(1.2) ** np.arange(8, dtype=np.float32)) ** 2).astype(np.float32)


def rot(rv):
    rv = np.asarray(rv, np.float64)
    th = np.linalg.norm(rv)
    if th == 0:
        return np.eye(3)
    k = rv / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def make(seed, n=64, cam=0, depth=(4.0, 60.0), spread=(20.0, 4.0), offset=(0.0, 0.0), stereo_frac=0.7, rv=(0.01, -0.03, 0.005),
         t=(0.12, -0.02, -0.55), start="identity", start_drv=(0.0, 0.0, 0.0), start_dt=(0.0, 0.0, 0.0), bad_frac=0.15, noise_px=0.5,
         has_frac=0.8, unrelated=False):
    """Points at `depth` in front of a camera at (rot(rv) | t), `spread` metres either side of `offset`; level-scaled noise; a
    fraction of gross outliers; `unrelated`: observations that have nothing to do with the points.  The start pose is the
    identity, or the truth moved by (start_drv, start_dt)."""
    rng = np.random.default_rng(seed)
    c = CAMS[cam]
    R, t = rot(rv), np.asarray(t, np.float64)
    z = rng.uniform(depth[0], depth[1], n)
    Xc = np.stack([offset[0] + rng.uniform(-spread[0], spread[0], n), offset[1] + rng.uniform(-spread[1], spread[1], n), z], 1)
    Xw = (Xc - t) @ R
    u = c["fx"] * Xc[:, 0] / z + c["cx"]
    v = c["fy"] * Xc[:, 1] / z + c["cy"]
    ur = u - c["bf"] / z
    lvl = rng.integers(0, 8, n)
    nz = rng.normal(0, noise_px, (n, 3)) * (1.2 ** lvl)[:, None]
    u, v, ur = u + nz[:, 0], v + nz[:, 1], ur + nz[:, 2]
    mono = (rng.random(n) >= stereo_frac) | (ur < 0)
    ur = np.where(mono, -1.0, ur)
    bad = rng.random(n) < bad_frac
    u = u + np.where(bad, rng.uniform(20, 40, n) * rng.choice([-1, 1], n), 0)
    if unrelated:
        u, v = rng.uniform(0, 1200, n), rng.uniform(0, 370, n)
    keys = np.zeros(n, O.KP_DTYPE)
    keys["x"], keys["y"], keys["octave"] = u, v, lvl
    has = (rng.random(n) < has_frac).astype(np.uint8)
    T0 = np.eye(4, dtype=np.float32)
    if start == "near":
        T0[:3, :3] = (rot(start_drv) @ R).astype(np.float32)
        T0[:3, 3] = (t + np.asarray(start_dt)).astype(np.float32)
    return dict(keys=keys, ur=ur.astype(np.float32), has=has, Xw=Xw.astype(np.float32), T0=T0, cam=cam)


# name -> arguments of make().  Chosen by a seeded search over camera, depth range (0.05 to 60 m), lateral spread (0.1 to 20 m per
# axis, with an offset), stereo fraction and rotation, keeping the smallest set whose traces cover tests/golden/pose_census.json's
# required items and that meets the three conditions of test_pose_census.py.
SCENES = {
    'default': dict(seed=201, n=200),
    'contaminated': dict(seed=202, n=300, bad_frac=0.4),
    'turned_x': dict(seed=203, n=200, rv=(3.1, 0.05, -0.02), t=(0.12, -0.02, -0.55), start='near', start_dt=(0.1, 0.0, 0.0)),
    'turned_y': dict(seed=204, n=200, rv=(0.04, 3.12, 0.03), t=(0.12, -0.02, -0.55), start='near', start_dt=(0.0, 0.1, 0.0)),
    'turned_z': dict(seed=205, n=200, rv=(-0.03, 0.02, 3.13), t=(0.12, -0.02, -0.55), start='near', start_dt=(0.0, 0.0, 0.1)),
    'far_start': dict(seed=206, n=257, rv=(0.2, -0.1, 0.15), t=(0.8, -0.3, 0.9)),
    'close_other_camera': dict(seed=207, n=64, cam=1, depth=(0.3, 3.0), spread=(0.5, 0.3), t=(0.05, -0.02, 0.1)),
    'search_2249': dict(seed=2249, n=12, cam=2, depth=(0.05, 0.25), spread=(0.62, 0.11), offset=(0.0, 0.0), stereo_frac=1.0, rv=(-0.2, -0.22, 0.19), t=(-0.29, 0.42, -0.26), start='near', start_dt=(0.136, -0.003, -0.162), start_drv=(-0.032, 0.025, -0.018), bad_frac=0.15, noise_px=0.0, has_frac=0.8),
    'search_1234': dict(seed=1234, n=100, cam=2, depth=(0.05, 5.0), spread=(0.14, 13.84), offset=(-3.6, 3.0), stereo_frac=1.0, rv=(3.1, 0.05, -0.02), t=(0.47, 0.38, -0.29), start='near', start_dt=(-0.066, -0.02, -0.021), start_drv=(-0.011, -0.018, 0.015), bad_frac=0.15, noise_px=1.5, has_frac=0.8),
    'search_1018': dict(seed=1018, n=12, cam=1, depth=(0.05, 0.1), spread=(0.14, 0.14), offset=(0.0, 0.0), stereo_frac=0.0, rv=(0.04, 3.12, 0.03), t=(0.47, 0.03, 0.19), start='near', start_dt=(-0.008, 0.007, -0.013), start_drv=(-0.001, 0.003, 0.002), bad_frac=0.15, noise_px=0.5, has_frac=0.8),
    'search_1071': dict(seed=1071, n=12, cam=2, depth=(1.0, 5.0), spread=(1.93, 7.03), offset=(0.0, 0.0), stereo_frac=1.0, rv=(0.04, 3.12, 0.03), t=(0.26, -0.34, 0.08), start='near', start_dt=(0.022, 0.073, -0.015), start_drv=(-0.016, -0.003, 0.013), bad_frac=0.4, noise_px=0.0, has_frac=0.8),
    'search_1086': dict(seed=1086, n=12, cam=0, depth=(0.3, 30.0), spread=(0.9, 0.92), offset=(-1.1, 0.6), stereo_frac=1.0, rv=(-0.03, 0.02, 3.13), t=(0.34, -0.06, -0.3), start='near', start_dt=(-0.031, 0.092, 0.02), start_drv=(0.013, 0.015, 0.002), bad_frac=0.15, noise_px=1.5, has_frac=1.0),
    'search_79': dict(seed=79, n=12, has_frac=0.12),
}


def scenes():
    return {name: make(**kw) for name, kw in SCENES.items()}


def run_oracle(s, T0=None, outlier=None, order=None):
    """The oracle on scene s (optionally with its slots permuted by `order`; flags come back in the scene's own order).
    Returns (T, outlier, n_inliers, trace)."""
    c = CAMS[s["cam"]]
    idx = np.arange(len(s["keys"])) if order is None else np.asarray(order)
    T, out, n = O.pose_optimization(s["T0"] if T0 is None else T0, s["keys"][idx], s["ur"][idx], s["has"][idx], s["Xw"][idx], INV_SIGMA2,
                                    c["fx"], c["fy"], c["cx"], c["cy"], c["bf"], None if outlier is None else np.asarray(outlier)[idx])
    tr = O.pose_trace()
    back = np.empty_like(out)
    back[idx] = out
    return T, back, n, tr


REQUIRED = ["branch_trace", "branch_0", "branch_1", "branch_2"] + ["exchange_%d_%d" % (k, c) for k in range(5) for c in range(k + 1, 6)] + [
    "rejected_trial", "stop_no_progress", "round_no_active_edge", "ne_below_10", "ne_below_3", "exp_small", "huber_above", "huber_below",
    "outlier_returned", "round_ends_rejected"]
RECORDED = ["stop_qmax", "stop_rho_zero", "stop_iterations", "solve_not_positive", "q11_witnesses"]


def items(tr):
    """The census items one trace shows: {item: count}."""
    d = {}
    if tr["ne"] >= 3:
        d[["branch_trace", "branch_0", "branch_1", "branch_2"][tr["input_branch"]]] = 1
    for k, c in tr["exchanges"]:
        d["exchange_%d_%d" % (k, c)] = 1
    d["rejected_trial"] = tr["rejected"]
    for name, stop in (("stop_no_progress", "no_progress"), ("stop_qmax", "qmax"), ("stop_rho_zero", "rho_zero"), ("stop_iterations", "iterations")):
        d[name] = tr["stop"].count(stop)
    d["round_no_active_edge"] = tr["rounds_no_active"]
    d["ne_below_10"] = int(3 <= tr["ne"] < 10)
    d["ne_below_3"] = int(tr["ne"] < 3)
    for k in ("exp_small", "huber_above", "huber_below", "outlier_returned", "q11_witnesses"):
        d[k] = tr[k]
    d["round_ends_rejected"] = tr["rounds_end_rejected"]
    d["solve_not_positive"] = tr["solves_not_positive"]
    return {k: int(v) for k, v in d.items() if v}


def census():
    """{"scenes": {name: items}, "union": {item: number of scenes that show it}} over SCENES, from the oracle."""
    per = {name: items(run_oracle(s)[3]) for name, s in scenes().items()}
    union = {}
    for it in per.values():
        for k in it:
            union[k] = union.get(k, 0) + 1
    return dict(scenes=per, union={k: union.get(k, 0) for k in REQUIRED + RECORDED})
