"""Seeded scenes of Optimizer::LocalBundleAdjustment for tests/test_lba_model.py (CPU) and tests/test_lba_device.py (GPU), with the
float64 model's answer (tests/lba_model.py) computed once per process and shared.

Geometry: keyframes on a line of at most 3.5 m looking down +z with small rotations, points 4 .. 10 m in front of them (every coordinate
below 16 m, so one float ulp stays under 1e-6), the camera of tests.device_arrays.context().  Observations are the projections of the
ground truth plus noise of 0.7 px times the level's scale factor; a tenth are gross outliers (20 .. 50 px).  Local keyframes start
1 cm / 0.01 rad off, points 3 cm off.  Every scene fixes its gauge with role-3 or role-2 keyframes that carry stereo edges (two with
mono edges in `mono`).  Every scene keeps 1 % distance from 5.991 / 7.815 and DEPTH_MARGIN from the camera plane at BOTH
classifications (asserted in tests/test_lba_model.py; a scene that misses is reseeded here, never exempted).

Boundary scenes of the kernel (orbslam2_amd/csrc/orbfe_lba.hip, LBA_THREADS = 512, 8 waves): points_511/512/513 (the stride of the
per-point passes), edges_511/512/513 (the stride of the per-edge passes and the chunks of the counting sort), free_7/8/9 (the waves'
stride over the free keyframes), free_20/21/22 (ORBFE_LBA_LDS_KEYFRAMES - 1, 0, + 1: free_22 is `reduced_hbm`), views_63/64/65 (a point
observed by that many keyframes, a free one last: the Schur rows fetch a point's list 64 entries at a time) and kf_edges_63/64/65 (a
free keyframe with that many edges, all at level 0 in both rounds: both keyframe walks fetch a keyframe's edges 64 at a time).
"""
import functools

import numpy as np

from tests import lba_model as M
from tests import pose_blocks_model as PB
from tests.sim3_opt_scenes import INV_SIGMA2, KP_DTYPE, NLEVELS

CAM = (500.0, 500.0, 320.0, 240.0, 50.0)    # tests/test_matchers.py: FX, FY, CX, CY, BF
DEPTH_MARGIN = 0.05
LDS_KEYFRAMES = 21                          # ORBFE_LBA_LDS_KEYFRAMES
L, H, F, S = M.LOCAL, M.LOCAL_HELD, M.FIXED, M.SKIP


def _project(T, X):
    P = T[:3, :3] @ X + T[:3, 3]
    return np.array([P[0] / P[2] * CAM[0] + CAM[2], P[1] / P[2] * CAM[1] + CAM[3], P[0] / P[2] * CAM[0] + CAM[2] - CAM[4] / P[2]]), P[2]


def make(seed, roles, n_pts=40, slots=64, views=4, mono=0.3, outliers=0.1, noise=1.0, spacing=0.4, behind=0, behind_kfs=(), behind_only=(), rows=False,
         n_obs=None, wide=0, exact=None):
    """wide = N: one more point, straight ahead of the middle of the line, observed by N keyframes, a local one last in its list.
    exact = (k, N): keyframe k observes exactly N points, with 0.3 of the noise and no outlier, so that all N edges stay at level 0."""
    rng = np.random.default_rng(seed)
    roles = np.array(roles, np.uint8)
    n_kfs = len(roles)
    Tgt = np.zeros((n_kfs, 4, 4))
    for k in range(n_kfs):
        Tgt[k] = np.eye(4)
        Tgt[k][:3, :3] = PB.rot(rng.uniform(-0.05, 0.05, 3))
        Tgt[k][:3, 3] = -Tgt[k][:3, :3] @ np.array([spacing * k, rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)])
    span = spacing * (n_kfs - 1)
    keys = [np.zeros(slots, KP_DTYPE) for _ in range(n_kfs)]
    ur = [np.full(slots, -1.0, np.float32) for _ in range(n_kfs)]
    for k in range(n_kfs):
        keys[k]["x"], keys[k]["y"], keys[k]["octave"] = rng.uniform(20, 620, slots), rng.uniform(20, 460, slots), rng.integers(0, NLEVELS, slots)
    order = [list(rng.permutation(slots)) for _ in range(n_kfs)]
    sig = 0.7 * np.float64(1.2) ** np.arange(NLEVELS)
    Xgt, off, okf, oidx = [], [0], [], []
    n_ord = n_pts + (1 if wide else 0)
    kx, kn, kcount = (exact[0], exact[1], 0) if exact else (-1, 0, 0)
    for q in range(n_ord + behind):
        is_behind, is_wide = q >= n_ord, bool(wide) and q == n_pts
        for _ in range(1000):
            X = np.array([rng.uniform(-1.0, span + 1.0), rng.uniform(-1.5, 1.5), rng.uniform(4.0, 10.0) * (-1 if is_behind else 1)])
            if is_wide:
                X = np.array([span / 2, 0.0, 8.0])
            pool = behind_kfs if is_behind else [k for k in range(n_kfs) if k not in behind_only and not (is_wide and k == kx)]
            uv = {k: _project(Tgt[k], X)[0] for k in pool if order[k]}
            cand = [k for k in uv if 20 < uv[k][0] < 620 and 20 < uv[k][1] < 460 and uv[k][2] > 0]
            if len(cand) >= (len(behind_kfs) if is_behind else min(views, 2)):
                break
        else:
            raise AssertionError("no place for point %d" % q)
        seen = list(rng.permutation(cand))[:len(cand) if is_behind else views]
        if is_wide:
            assert len(cand) >= wide
            local = [k for k in cand if roles[k] == L][0]
            seen = [k for k in rng.permutation(cand) if k != local][:wide - 1] + [local]
        elif exact and not is_behind:
            seen = [k for k in seen if k != kx]
            if kcount < kn and kx in cand:
                seen, kcount = [kx] + seen[:views - 1], kcount + 1
        Xgt.append(X)
        for k in seen:
            i = order[k].pop()
            uvr, _ = _project(Tgt[k], X)
            o = int(keys[k]["octave"][i])
            quiet = is_wide or k == kx
            uvr = uvr + rng.normal(0, noise * (0.3 if quiet else 1.0) * sig[o], 3)
            if not is_behind and not quiet and rng.uniform() < outliers:
                a = rng.uniform(0, 2 * np.pi)
                uvr[:2] += rng.uniform(20, 50) * np.array([np.cos(a), np.sin(a)])
            keys[k]["x"][i], keys[k]["y"][i] = uvr[0], uvr[1]
            ur[k][i] = -1.0 if (is_behind or rng.uniform() < mono) else uvr[2]
            okf.append(k)
            oidx.append(i)
        off.append(len(okf))
    Xgt = np.array(Xgt).reshape(-1, 3)
    Tcw = np.zeros((n_kfs, 16), np.float32)
    for k in range(n_kfs):
        T = Tgt[k]
        if roles[k] == L:
            D = np.eye(4)
            D[:3, :3], D[:3, 3] = PB.rot(rng.normal(0, 0.006, 3)), rng.normal(0, 0.006, 3)
            T = D @ T
        if roles[k] == H:             # a drifted float row, 1e-4 off orthonormal: its round trip through the quaternion is visible
            T = T.copy()
            T[:3, :3] *= 1.0001
        Tcw[k] = T.astype(np.float32).reshape(16)
    assert kcount == kn
    n_all = n_ord + behind
    pos0 = (Xgt + rng.normal(0, 0.03, Xgt.shape) * (np.arange(n_all) < n_ord)[:, None] + rng.normal(0, 0.005, Xgt.shape)).astype(np.float32)
    if rows:
        n_rows = n_all + 17
        row = rng.permutation(n_rows)[:n_all].astype(np.int32)
        pos = rng.uniform(-5, 5, (n_rows, 3)).astype(np.float32)
        pos[row] = pos0
    else:
        n_rows, row, pos = n_all, None, pos0
    off, okf, oidx = np.array(off, np.int32), np.array(okf, np.int32), np.array(oidx, np.int32)
    if n_obs is not None:         # cut the observation arrays to an exact length: the last lists get shorter or empty
        assert n_obs <= len(okf)
        off, okf, oidx = np.minimum(off, n_obs).astype(np.int32), okf[:n_obs], oidx[:n_obs]
    return dict(kfs=list(zip(keys, ur)), role=roles, Tcw=Tcw, row=row, n_rows=n_rows, obs_off=off, obs_kf=okf, obs_idx=oidx, pos=pos,
                max_free=int((roles == L).sum()), Tgt=Tgt, Xgt=Xgt)


MIXED = dict(roles=[L, F, L, H, L, F])
SPECS = {
    "mixed": dict(seed=101, **MIXED),
    "mono": dict(seed=2, roles=[L, F, L, F, L], mono=1.0),
    "stereo": dict(seed=3, roles=[L, L, F, L, F], mono=0.0),
    "behind": dict(seed=4, roles=[L, F, L, F, L], behind=3, behind_kfs=(0, 1, 3)),
    "orphans": dict(seed=5, roles=[L, F, L, F, L, L], n_pts=30, behind=4, behind_kfs=(1, 3, 5), behind_only=(5,)),   # keyframe 5 sees the behind points only
    "stale": dict(seed=6, roles=[L, F, L, F], n_pts=20, noise=0.3),   # round 2 ends on ten rejected trials
    "skip": dict(seed=7, roles=[L, S, L, F, H, F]),
    "rows": dict(seed=8, rows=True, **MIXED),
    "reduced_hbm": dict(seed=9, roles=[F] + [L] * (LDS_KEYFRAMES + 1) + [F], n_pts=70, slots=32, views=5, spacing=0.15),
    "free_20": dict(seed=10, roles=[F] + [L] * (LDS_KEYFRAMES - 1) + [F], n_pts=70, slots=32, views=5, spacing=0.15),
    "free_21": dict(seed=111, roles=[F] + [L] * LDS_KEYFRAMES + [F], n_pts=70, slots=32, views=5, spacing=0.15),
    "free_7": dict(seed=12, roles=[F] + [L] * 7 + [F], n_pts=40, slots=48, spacing=0.3),
    "free_8": dict(seed=13, roles=[F] + [L] * 8 + [F], n_pts=40, slots=48, spacing=0.3),
    "free_9": dict(seed=14, roles=[F] + [L] * 9 + [F], n_pts=40, slots=48, spacing=0.3),
    "points_511": dict(seed=15, roles=[L, F, L, F, L], n_pts=511, slots=512, views=2),
    "points_512": dict(seed=16, roles=[L, F, L, F, L], n_pts=512, slots=512, views=2),
    "points_513": dict(seed=617, roles=[L, F, L, F, L], n_pts=513, slots=512, views=2),
    "edges_511": dict(seed=18, roles=[L, F, L, F, L], n_pts=130, slots=160, n_obs=511),
    "edges_512": dict(seed=19, roles=[L, F, L, F, L], n_pts=130, slots=160, n_obs=512),
    "edges_513": dict(seed=20, roles=[L, F, L, F, L], n_pts=130, slots=160, n_obs=513),
    "views_63": dict(seed=21, roles=[L, L, L] + [F] * 63, n_pts=30, slots=40, spacing=0.03, wide=63),
    "views_64": dict(seed=22, roles=[L, L, L] + [F] * 63, n_pts=30, slots=40, spacing=0.03, wide=64),
    "views_65": dict(seed=23, roles=[L, L, L] + [F] * 63, n_pts=30, slots=40, spacing=0.03, wide=65),
    "kf_edges_63": dict(seed=24, roles=[L, F, L, F, L], n_pts=100, slots=128, exact=(2, 63)),
    "kf_edges_64": dict(seed=525, roles=[L, F, L, F, L], n_pts=100, slots=128, exact=(2, 64)),
    "kf_edges_65": dict(seed=326, roles=[L, F, L, F, L], n_pts=100, slots=128, exact=(2, 65)),
}
FAULTY = ("faulty_obs_kf", "faulty_obs_idx", "faulty_octave", "faulty_role", "faulty_row", "faulty_offset", "faulty_descending")
EMPTY = ("empty", "all_skipped")
DEVICE_SCENES = tuple(SPECS) + FAULTY + EMPTY


def _copy(s):
    out = dict(s)
    out["kfs"] = [(k.copy(), u.copy()) for k, u in s["kfs"]]
    for f in ("role", "Tcw", "obs_off", "obs_kf", "obs_idx", "pos"):
        out[f] = s[f].copy()
    out["row"] = None if s["row"] is None else s["row"].copy()
    return out


@functools.lru_cache(maxsize=None)
def _scene(name):
    if name in SPECS:
        return make(**SPECS[name])
    s = _copy(_scene("rows"))
    e = len(s["obs_kf"])
    if name == "faulty_obs_kf":
        s["obs_kf"][5], s["obs_kf"][e // 2] = len(s["role"]), -1
    elif name == "faulty_obs_idx":
        s["obs_idx"][7], s["obs_idx"][e // 3] = len(s["kfs"][0][0]), -1
    elif name == "faulty_octave":
        for j in (3, e - 2):
            s["kfs"][s["obs_kf"][j]][0]["octave"][s["obs_idx"][j]] = NLEVELS if j == 3 else -1
    elif name == "faulty_role":
        s["role"][4] = 7
        s["max_free"] = int((s["role"] == L).sum())
    elif name == "faulty_row":
        s["row"][2], s["row"][11] = s["n_rows"], -1
    elif name == "faulty_offset":
        s["obs_off"][0], s["obs_off"][-1] = -1, e + 5
    elif name == "faulty_descending":
        # one more point in front whose offsets descend, (off[1], 0): it is faulty and owns nothing; every entry keeps its one owner
        # (a descent that makes two lists overlap is outside the contract: include/orbfe.h)
        s["obs_off"] = np.concatenate([[s["obs_off"][1]], s["obs_off"]]).astype(np.int32)
        spare = np.setdiff1d(np.arange(s["n_rows"]), s["row"])[0]
        s["row"] = np.concatenate([[spare], s["row"]]).astype(np.int32)
    elif name == "empty":
        s["obs_off"], s["obs_kf"], s["obs_idx"], s["row"] = s["obs_off"][:1] * 0, s["obs_kf"][:0], s["obs_idx"][:0], s["row"][:0]
    elif name == "all_skipped":
        s["role"][:] = S
        s["max_free"] = 0
    else:
        raise KeyError(name)
    return s


def scene(name):
    """A fresh copy: a test may change its arrays."""
    return _copy(_scene(name))


def run_model(s, **kw):
    return M.local_bundle_adjustment(s["kfs"], s["role"], s["Tcw"], s["row"], s["n_rows"], s["obs_off"], s["obs_kf"], s["obs_idx"], s["pos"], CAM,
                                     INV_SIGMA2, NLEVELS, **kw)


@functools.lru_cache(maxsize=None)
def model(name):
    """The model's answer, computed once and left unchanged."""
    return run_model(_scene(name), max_free_kfs=_scene(name)["max_free"])
