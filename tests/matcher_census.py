"""Census of the seven projection matchers: which way every decision of the reference's loops goes on the inputs of the suite, and
the inputs that are built to reach what the existing scenes never reach.

The counters live in oracle/literal_matchers.py and oracle/literal_kf_matchers.py (an optional `census` dict that the literal
transcriptions increment; results are unchanged).  This module holds the inputs and three runners per matcher: the C oracle, the
literal transcription (with or without counters, on the reference's grid or on a grid that hands its windows over in a wrong
order), and -- in tests/test_gpu_matcher_census.py -- the HIP entry points.  tests/test_matcher_census.py holds the literal
transcription against the oracle exactly, which is what makes the counters trustworthy.

Matchers (reference src/ORBmatcher.cc):
  last             SearchByProjection(CurrentFrame, LastFrame, th, bMono)      :1324-1466
  points           Frame::isInFrustum + SearchByProjection(F, vpMapPoints, th)  src/Frame.cc:256-315, :43-135
  kf               SearchByProjection(CurrentFrame, KeyFrame, ...)              :1468-1595
  fuse             Fuse(KeyFrame*, vpMapPoints, th)                             :821-971
  sim3_projection  SearchByProjection(KeyFrame*, Scw, ...)                      :285-398
  sim3_fuse        Fuse(KeyFrame*, Scw, ...)                                    :973-1096
  by_sim3          SearchBySim3                                                 :1098-1322
"""
from __future__ import annotations

import numpy as np

from oracle import literal_kf_matchers as LK
from oracle import literal_matchers as LM
from oracle import oracle as O
from tests import test_matchers as TM

W, H, FX, FY, CX, CY, BF, NL, LOG_SF, CAM = TM.W, TM.H, TM.FX, TM.FY, TM.CX, TM.CY, TM.BF, TM.NL, TM.LOG_SF, TM.CAM
CAMT = (FX, FY, CX, CY, BF, BF / FX)
FRAME_BOUNDS = (0.0, float(W), 0.0, float(H))
MATCHERS = ("last", "points", "kf", "fuse", "sim3_projection", "sim3_fuse", "by_sim3")
GOLDEN = "matcher_census.json"  # under tests/golden/


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def _points_of(s, rng, noise):
    """Normal, mfMaxDistance and mfMinDistance of a scene's map points as MapPoint computes them (src/MapPoint.cc:330-363): the
    points were created from the frame at the origin, at level `octave`."""
    n = len(s["pos"])
    dist0 = np.linalg.norm(s["pos"], axis=1).astype(np.float32)
    s["max_d"] = (dist0 * s["sf"][s["octave"]]).astype(np.float32)
    s["min_d"] = (s["max_d"] / s["sf"][NL - 1]).astype(np.float32)
    normal = (s["pos"] / dist0[:, None] + rng.normal(0, noise, (n, 3))).astype(np.float32)
    s["normal"] = (normal / np.linalg.norm(normal, axis=1, keepdims=True)).astype(np.float32)
    return s


def _finish(s, keyframe=False, sim3_scale=1.07):
    s.setdefault("desc", s.get("desc_last"))
    s.setdefault("has", s.get("cur_has_obs"))
    s["keyframe"] = keyframe
    s["inv_sigma2"] = s["ex"].inv_sigma2()
    Scw = s["T_cur"].copy(); Scw *= np.float32(sim3_scale)  # [sR | s t]: the same camera pose, the map scaled
    s["Scw"] = Scw
    return s


def _existing_kf_side(seed, bounds=None):
    """The scene of test_gpu_fuse / test_gpu_sim3_projection_matchers / test_gpu_keyframe_views_use_the_keyframes_integer_bounds
    (tests/test_matchers.py), same seed and draw order."""
    s = TM._scene(seed, n_last=1500, n_distract=400)
    rng = np.random.default_rng(seed)
    _points_of(s, rng, 0.45)
    if bounds is not None:
        for _ in range(3):
            rng.uniform(0, 1, 600)  # the three window-query draws of the keyframe-bounds test
        s["bounds"] = bounds
    s["kf_matched"] = (rng.random(len(s["k"])) < 0.1).astype(np.uint8)
    return _finish(s, keyframe=bounds is not None)


def _existing_tracking(seed, n_last=900):
    """Scenes of test_gpu_search_by_projection_last / _frustum_and_search_by_projection_points / _search_by_projection_kf."""
    s = TM._scene(seed, n_last=n_last)
    rng = s["rng"]
    n = len(s["pos"])
    if seed == 20:
        normal = s["pos"] / np.linalg.norm(s["pos"], axis=1, keepdims=True) + rng.normal(0, 0.35, (n, 3))
        s["normal"] = (normal / np.linalg.norm(normal, axis=1, keepdims=True)).astype(np.float32)
    dist0 = np.linalg.norm(s["pos"], axis=1).astype(np.float32)
    s["max_d"] = (dist0 * rng.uniform(0.9, 3.0, n)).astype(np.float32); s["min_d"] = (s["max_d"] / np.float32(1.2 ** 7)).astype(np.float32)
    s.setdefault("normal", (s["pos"] / dist0[:, None]).astype(np.float32))
    s["kf_matched"] = None
    return _finish(s)


def _roll(deg, t):
    """A rotation about the optical axis: the third row of [R|t] is (0, 0, 1, tz) exactly, so a point with z == -tz has depth 0."""
    a = np.deg2rad(deg)
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], np.float64)
    return np.concatenate([R, np.array(t, np.float64)[:, None]], axis=1).astype(np.float32)


def _back_project(T, u, v, z):
    """World point whose projection by [R|t] = T is (u, v) at depth z (double arithmetic; the float projection lands within 1e-3 px)."""
    T = T.astype(np.float64)
    pc = np.stack([(u - CX) * z / FX, (v - CY) * z / FY, z * np.ones_like(u)], axis=1)
    return ((pc - T[:, 3]) @ T[:, :3]).astype(np.float32)


def _project(T, pos):
    T = T.astype(np.float64)
    pc = (T[:, :3] @ pos.T.astype(np.float64)).T + T[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        return pc, FX * pc[:, 0] / pc[:, 2] + CX, FY * pc[:, 1] / pc[:, 2] + CY


def _map_points(rng, n, T_cur, sf, pos=None):
    if pos is None:
        u = rng.uniform(20, W - 20, n); v = rng.uniform(20, H - 20, n); z = rng.uniform(2.0, 40.0, n)
        pos = np.stack([(u - CX) * z / FX, (v - CY) * z / FY, z], axis=1).astype(np.float32)
    s = dict(pos=pos, octave=rng.integers(0, NL, n).astype(np.int32), angle=rng.uniform(0, 360, n).astype(np.float32),
             desc=rng.integers(0, 256, (n, 32)).astype(np.uint8), valid=(rng.random(n) < 0.85).astype(np.int32),
             obs=rng.integers(0, 3, n).astype(np.int32), T_last=TM._se3(0.0, [0, 0, 0]), T_cur=T_cur, sf=sf)
    return s


def _predicted_level(s):
    """MapPoint::PredictScale of every point seen from T_cur (double arithmetic: only used to give keypoints a plausible octave)."""
    T = s["T_cur"].astype(np.float64)
    ow = -T[:, :3].T @ T[:, 3]
    dist0 = np.linalg.norm(s["pos"].astype(np.float64), axis=1)
    dist1 = np.linalg.norm(s["pos"].astype(np.float64) - ow, axis=1)
    return s["octave"] + np.ceil(np.log(dist0 / np.maximum(dist1, 1e-9)) / np.log(1.2)).astype(np.int64), dist1


def _observe(s, rng, n_distract, skip=None):
    """The current frame of a scene: re-projections of the map points (jitter, bit flips, octave near the predicted level) and
    distractors, shuffled; the points listed in `skip` get no keypoint."""
    n = len(s["pos"])
    pc, uu, vv = _project(s["T_cur"], s["pos"])
    pred, dist1 = _predicted_level(s)
    keep = (rng.random(n) < 0.8) & (pc[:, 2] > 0.05) & (uu > -5) & (uu < W + 5) & (vv > -5) & (vv < H + 5)
    if skip is not None:
        keep &= ~np.isin(np.arange(n), skip)
    m = int(keep.sum())
    k = np.zeros(m + n_distract, O.KP_DTYPE); d = np.zeros((len(k), 32), np.uint8); ur = np.full(len(k), -1.0, np.float32)
    src = np.full(len(k), -1, np.int64); src[:m] = np.nonzero(keep)[0]
    k["x"][:m] = uu[keep] + rng.normal(0, 1.2, m); k["y"][:m] = vv[keep] + rng.normal(0, 1.2, m)
    k["octave"][:m] = np.clip(pred[keep] + rng.integers(-1, 2, m), 0, NL - 1)
    k["angle"][:m] = (s["angle"][keep] + rng.normal(0, 6, m)) % 360
    d[:m] = s["desc"][keep] ^ np.packbits(rng.random((m, 256)) < 0.07, axis=1, bitorder="little")
    has_r = rng.random(m) < 0.7
    ur[:m] = np.where(has_r, k["x"][:m] - BF / pc[keep, 2] + rng.normal(0, 0.8, m), -1.0)
    k["x"][m:] = rng.uniform(0, W, n_distract); k["y"][m:] = rng.uniform(0, H, n_distract)
    k["octave"][m:] = rng.integers(0, NL, n_distract); k["angle"][m:] = rng.uniform(0, 360, n_distract)
    d[m:] = rng.integers(0, 256, (n_distract, 32))
    k["size"] = 31; k["class_id"] = -1
    perm = rng.permutation(len(k))
    k, d, ur, src = k[perm], d[perm], ur[perm], src[perm]
    s.update(k=k, d=d, ur=ur, src=src, dist1=dist1)
    return s


def _complete(s, rng, bounds=FRAME_BOUNDS, keyframe=False, ex=None):
    """Everything else the seven matchers read: flags of the current keypoints, MapPoint fields, and the first keyframe of SearchBySim3
    (one keypoint per map point at the identity pose, its descriptor the map point's) with the second one's own map points."""
    n, nk = len(s["pos"]), len(s["k"])
    s["ex"] = ex or O.Extractor()
    s["bounds"] = bounds
    s.setdefault("has", (rng.random(nk) < 0.05).astype(np.uint8))
    s.setdefault("kf_matched", (rng.random(nk) < 0.1).astype(np.uint8))
    _points_of(s, rng, 0.45)
    _, u0, v0 = _project(s["T_last"], s["pos"])
    k1 = np.zeros(n, O.KP_DTYPE)
    k1["x"] = u0 + rng.normal(0, 0.8, n); k1["y"] = v0 + rng.normal(0, 0.8, n); k1["octave"] = s["octave"]; k1["angle"] = s["angle"]
    k1["size"] = 31; k1["class_id"] = -1
    s["k1"], s["d1"] = k1, s["desc"]
    src = s["src"]
    ok = src >= 0
    pos2 = np.zeros((nk, 3), np.float32); pos2[ok] = s["pos"][src[ok]]
    mx2 = np.ones(nk, np.float32); mx2[ok] = (s["dist1"][src[ok]] * s["sf"][s["k"]["octave"][ok]]).astype(np.float32)
    s["pts1"] = (s["pos"], s["max_d"], s["min_d"], s["desc"], s["valid"])
    s["pts2"] = (pos2, mx2, (mx2 / s["sf"][NL - 1]).astype(np.float32), s["d"], (ok & (rng.random(nk) < 0.85)).astype(np.int32))
    T2 = s["T_cur"].astype(np.float64)
    s["R12"] = T2[:, :3].T.astype(np.float32)                 # camera 1 is the world: X1 = R2^T (X2 - t2)
    s["t12"] = (-T2[:, :3].T @ T2[:, 3]).astype(np.float32)
    s["s12"] = np.float32(1.02)
    return _finish(s, keyframe=keyframe)


def _camera_scene(seed, T_cur, n_pts=500, n_distract=150, on_plane=0, bounds=FRAME_BOUNDS, keyframe=False, turned=0.0, swapped=0):
    """A cloud seen first from the origin and then from T_cur, which may stand anywhere: among the points, far behind, ...
    turned: share of the current keypoints with an unrelated orientation (the rotation histogram turns their matches away);
    swapped: so many keypoints of the second keyframe hold ANOTHER keypoint's map point (SearchBySim3's two directions disagree)."""
    rng = np.random.default_rng(seed)
    ex = O.Extractor()
    s = _map_points(rng, n_pts, T_cur, ex.scale_factors())
    if on_plane:  # a few valid points exactly on the plane z == 0 of the current camera (T_cur from _roll), off its axis
        s["pos"][:on_plane, 2] = -T_cur[2, 3]
        s["valid"][:on_plane] = 1
    _observe(s, rng, n_distract)
    if turned:
        t = rng.random(len(s["k"])) < turned
        s["k"]["angle"][t] = rng.uniform(0, 360, int(t.sum()))
    s = _complete(s, rng, bounds, keyframe, ex)
    if swapped:
        pos2, mx2, mn2, d2, v2 = s["pts2"]
        d2 = d2.copy()
        own = np.nonzero(s["src"] >= 0)[0]
        done = 0
        for j in own:
            other = [q for q in own if q != j and s["octave"][s["src"][q]] == s["octave"][s["src"][j]] and s["k"]["octave"][q] == s["k"]["octave"][j]]
            if done == swapped or not other:
                continue
            q = other[int(rng.integers(len(other)))]
            pos2[j], mx2[j], mn2[j], d2[j], v2[j] = pos2[q], mx2[q], mn2[q], s["d"][q], 1
            done += 1
        s["pts2"] = (pos2, mx2, mn2, d2, v2)
    return s


def _tie_scene(seed, n_clusters=160, n_plain=120, n_filler=0):
    """Clusters of two keypoints at the SAME Hamming distance from their map point (bit-identical descriptors, or two different ones
    equally far), placed around a cell corner (bx, by) = (10 c + 5, 10 r + 5) of the frame grid (10 x 10 px cells; PosInGrid rounds, so
    that is where four cells meet) that the point projects onto, one cluster kind after the other:
      kind 0  both in cell (c, r);
      kind 1  cells (c, r) and (c, r + 1) of one column, the LOWER keypoint index in the later row;
      kind 2  cells (c, r + 1) and (c + 1, r): two columns, the LOWER index in the later column and the earlier row.
    The reference's loop takes the first minimum in GetFeaturesInArea order (cell x, cell y, keypoint index): kind 1 and 2 tell it
    from `lowest keypoint index`, kind 2 from a cell-y-major traversal.  n_filler keypoints in the strip y < 50 push the cluster
    keypoints' indices beyond 32768; half of the corners lie at c >= 32 and r >= 32."""
    rng = np.random.default_rng(seed)
    ex = O.Extractor()
    T_cur = TM._se3(2.0, [0.02, -0.01, -0.3])
    nc = n_clusters
    c = np.where(np.arange(nc) % 2 == 0, rng.integers(3, 30, nc), rng.integers(33, 61, nc))
    r = np.where(np.arange(nc) % 2 == 0, rng.integers(10, 30, nc), rng.integers(33, 45, nc))
    cr = sorted({(int(a), int(b)) for a, b in zip(c, r)})  # distinct corners
    # corners at least 4 cells apart, so that no cluster lies in another one's window (at most +-26 px)
    picked = []
    for a, b in cr:
        if all(abs(a - p) > 3 or abs(b - q) > 3 for p, q in picked):
            picked.append((a, b))
    nc = len(picked)
    bx = np.array([10.0 * a + 5 for a, _ in picked]); by = np.array([10.0 * b + 5 for _, b in picked])
    pos_c = _back_project(T_cur, bx, by, rng.uniform(4.0, 30.0, nc))
    s = _map_points(rng, nc + n_plain, T_cur, ex.scale_factors())
    s["pos"][:nc] = pos_c
    s["valid"][:nc] = 1
    s["obs"][:nc] = 1
    # ordinary keypoints away from the clusters: their map points are points nc .. ; the cluster points get none from _observe
    _observe(s, rng, 60, skip=np.arange(nc))
    far = np.ones(len(s["k"]), bool)
    for x, y in zip(bx, by):
        far &= (np.abs(s["k"]["x"] - x) > 40) | (np.abs(s["k"]["y"] - y) > 40)
    if n_filler:
        far &= s["k"]["y"] > 95  # and out of reach of the filler strip
    base_k, base_d, base_ur, base_src = s["k"][far], s["d"][far], s["ur"][far], s["src"][far]
    offsets = {0: ((-1.2, -1.2), (-0.8, -0.8)), 1: ((-1.0, 1.0), (-1.0, -1.0)), 2: ((1.0, -1.0), (-1.0, 1.0))}  # (lower index, higher index)
    lo_k = np.zeros(nc, O.KP_DTYPE); hi_k = np.zeros(nc, O.KP_DTYPE)
    lo_d = np.zeros((nc, 32), np.uint8); hi_d = np.zeros((nc, 32), np.uint8)
    for i in range(nc):
        kind = i % 3
        nbits = 0 if i % 2 == 0 else int(rng.integers(1, 41))  # Hamming distance of both keypoints to the map point: 0, or 1 .. 40
        for kk, dd, (ox, oy), same in ((lo_k, lo_d, offsets[kind][0], True), (hi_k, hi_d, offsets[kind][1], i % 4 == 1)):
            kk["x"][i] = bx[i] + ox; kk["y"][i] = by[i] + oy
            kk["octave"][i] = s["octave"][i]; kk["angle"][i] = s["angle"][i]
            bits = np.zeros(256, bool)
            bits[(np.arange(nbits) if same else 255 - np.arange(nbits))] = True  # two different descriptors, equally far
            dd[i] = s["desc"][i] ^ np.packbits(bits, bitorder="little")
    for kk in (lo_k, hi_k):
        kk["size"] = 31; kk["class_id"] = -1
    fill_k = np.zeros(n_filler, O.KP_DTYPE)
    fill_k["x"] = rng.uniform(0, W, n_filler); fill_k["y"] = rng.uniform(0, 50, n_filler); fill_k["octave"] = rng.integers(0, NL, n_filler)
    fill_k["angle"] = rng.uniform(0, 360, n_filler); fill_k["size"] = 31; fill_k["class_id"] = -1
    fill_d = rng.integers(0, 256, (n_filler, 32)).astype(np.uint8)
    # index layout: [lower-index halves | ordinary | filler | higher-index halves]: with the filler the higher halves sit above 32768
    s["k"] = np.concatenate([lo_k, base_k, fill_k, hi_k]); s["d"] = np.concatenate([lo_d, base_d, fill_d, hi_d])
    s["ur"] = np.concatenate([np.full(nc, -1.0, np.float32), base_ur, np.full(n_filler, -1.0, np.float32), np.full(nc, -1.0, np.float32)])
    s["src"] = np.concatenate([np.arange(nc), base_src, np.full(n_filler, -1), np.arange(nc)])
    nk = len(s["k"])
    cluster = np.zeros(nk, bool); cluster[:nc] = True; cluster[nk - nc:] = True
    s["has"] = ((rng.random(nk) < 0.05) & ~cluster).astype(np.uint8)
    s["kf_matched"] = ((rng.random(nk) < 0.1) & ~cluster).astype(np.uint8)
    s["n_clusters"] = nc
    s = _complete(s, rng, ex=ex)
    s["pts2"][4][cluster] = 1  # both keypoints of a cluster hold the cluster's map point in the second keyframe
    return s


def _overflow_scene(seed=7):
    """72 map points: 24 project into a blob of 700 keypoints (windows of several hundred candidates, above the 256 the top-K stage
    holds), 24 into empty image, and 24 are copies of the first 24 -- where the original has Observations() == 0 its copy takes the
    same keypoint again and the reference counts both.  The windows sum to far more than 64 per query, the first size of the
    device's candidate list."""
    rng = np.random.default_rng(seed)
    ex = O.Extractor()
    T_cur = TM._se3(2.0, [0.02, -0.01, -0.3])
    n = 48
    u = np.concatenate([rng.uniform(305, 335, 24), rng.uniform(60, 580, 24)]); v = np.concatenate([rng.uniform(285, 315, 24), rng.uniform(60, 140, 24)])
    pos = _back_project(T_cur, u, v, rng.uniform(6.0, 25.0, n))
    s = _map_points(rng, n, T_cur, ex.scale_factors(), pos=pos)
    s["octave"][:] = 3; s["valid"][:] = 1; s["valid"][5] = 0
    s["obs"][:24] = np.arange(24) % 2
    for key in ("pos", "octave", "angle", "desc", "valid", "obs"):
        s[key] = np.concatenate([s[key], s[key][:24]])
    nb = 700
    k = np.zeros(nb, O.KP_DTYPE)
    k["x"] = rng.uniform(300, 340, nb); k["y"] = rng.uniform(280, 320, nb); k["octave"] = rng.integers(3, 5, nb); k["angle"] = rng.uniform(0, 360, nb)
    k["size"] = 31; k["class_id"] = -1
    d = rng.integers(0, 256, (nb, 32)).astype(np.uint8)
    src = np.full(nb, -1, np.int64)
    for i in range(24):  # one near copy of every blob point's descriptor, next to its projection
        k["x"][i] = u[i] + rng.normal(0, 0.7); k["y"][i] = v[i] + rng.normal(0, 0.7); k["angle"][i] = s["angle"][i]
        d[i] = s["desc"][i] ^ np.packbits(rng.random(256) < 0.05, bitorder="little"); src[i] = i
    perm = rng.permutation(nb)
    s.update(k=k[perm], d=d[perm], ur=np.full(nb, -1.0, np.float32), src=src[perm], dist1=_predicted_level(s)[1])
    return _complete(s, rng, ex=ex)


# name -> (builder, {matcher: parameters}, what the input is there for).  Parameters: last (th, mono, check_ori); points (th, nnratio);
# kf (th, ORBdist, check_ori); fuse (th, stereo); sim3_projection / sim3_fuse / by_sim3 (th,)
_ALL = {"last": (7.0, False, True), "points": (3.0, 0.8), "kf": (10.0, 100, True), "fuse": (3.0, True), "sim3_projection": (10.0,),
        "sim3_fuse": (4.0,), "by_sim3": (7.5,)}
_TIE = {"last": (7.0, False, True), "points": (3.0, 0.8), "kf": (10.0, 100, True), "fuse": (3.0, True), "sim3_projection": (4.0,),
        "sim3_fuse": (4.0,), "by_sim3": (7.5,)}
INPUTS = {
    # scenes the GPU suite already had (tests/test_matchers.py), under their seeds
    "fuse_40": (lambda: _existing_kf_side(40), {"fuse": (3.0, True)}, "existing input"),
    "fuse_41": (lambda: _existing_kf_side(41), {"fuse": (2.5, False)}, "existing input"),
    "fuse_42": (lambda: _existing_kf_side(42), {"fuse": (6.0, True)}, "existing input"),
    "sim3_50": (lambda: _existing_kf_side(50), {"sim3_projection": (10.0,)}, "existing input"),
    "sim3_51": (lambda: _existing_kf_side(51), {"sim3_projection": (4.0,)}, "existing input"),
    "sim3_52": (lambda: _existing_kf_side(52), {"sim3_fuse": (4.0,)}, "existing input"),
    "sim3_53": (lambda: _existing_kf_side(53), {"sim3_fuse": (10.0,)}, "existing input"),
    "kfbounds_71": (lambda: _existing_kf_side(71, TM.KF_BOUNDS), {"fuse": (3.0, True), "sim3_projection": (6.0,), "sim3_fuse": (6.0,)},
                    "existing input: integer bounds of a keyframe"),
    "track_10": (lambda: _existing_tracking(10), {"last": (7.0, False, True)}, "existing input"),
    "track_13": (lambda: _existing_tracking(13), {"last": (3.0, False, True)}, "existing input"),
    "track_20": (lambda: _existing_tracking(20, 1500), {"points": (3.0, 0.8)}, "existing input"),
    "track_30": (lambda: _existing_tracking(30), {"kf": (10.0, 100, True)}, "existing input"),
    # new
    "among": (lambda: _camera_scene(101, _roll(3.0, [0.3, -0.2, -12.0]), on_plane=6), _ALL,
              "camera among the points: z < 0, z == 0, too near, level clamped at nlevels - 1"),
    "retreat": (lambda: _camera_scene(102, _roll(-2.0, [-0.2, 0.1, 9.0]), turned=0.3), _ALL,
                "camera far behind its first pose: too far; a third of the keypoints turned: the rotation histogram rejects"),
    "among_kfbounds": (lambda: _camera_scene(103, _roll(-4.0, [-0.4, 0.3, -10.0]), on_plane=4, bounds=TM.KF_BOUNDS, keyframe=True),
                       {m: _ALL[m] for m in ("fuse", "sim3_projection", "sim3_fuse", "by_sim3")},
                       "the same gates behind the integer bounds of a keyframe: every single-sided bound"),
    "sideways": (lambda: _camera_scene(104, TM._se3(1.0, [0.25, 0.0, 0.03]), n_pts=400, swapped=60),
                 {"last": (14.0, False, False), "points": (1.0, 0.8), "kf": (3.0, 64, False), "by_sim3": (3.0,)},
                 "neither forward nor backward; th == 1; no rotation check; SearchBySim3's two directions disagree"),
    "tie": (lambda: _tie_scene(201), _TIE, "Hamming ties that decide accepted matches, three kinds"),
    "tie_wide": (lambda: _tie_scene(202, n_filler=33500), _TIE, "the same with keypoint indices above 32768 and cells beyond 32"),
    "overflow": (_overflow_scene, {"last": (15.0, False, False), "points": (5.0, 0.8), "kf": (15.0, 100, False), "fuse": (12.0, False),
                                   "sim3_projection": (12.0,), "sim3_fuse": (12.0,)},
                 "windows that sum to more than 64 candidates per query, one above 256 next to empty ones"),
}
EXISTING = tuple(n for n, v in INPUTS.items() if v[2].startswith("existing input"))
CASES = [(name, m) for name, v in INPUTS.items() for m in MATCHERS if m in v[1]]

_BUILT = {}


def build(name):
    if name not in _BUILT:
        _BUILT[name] = INPUTS[name][0]()
    return _BUILT[name]


# ---------------------------------------------------------------------------------------------------------------------
# runners
# ---------------------------------------------------------------------------------------------------------------------
def _ur(s, matcher, p):
    if matcher == "last":
        return None if p[1] else s["ur"]
    if matcher == "fuse":
        return s["ur"] if p[1] else None
    return None if matcher == "kf" else s["ur"]


def oracle_frustum(s):
    return O.is_in_frustum(s["T_cur"], CAM, s["bounds"], s["pos"], s["normal"], s["max_d"], s["min_d"], 0.5, LOG_SF, NL)


def oracle_run(matcher, s, p):
    """(matches, count) of the C oracle; the KeyFrame-side matchers always read a keyframe's grid (integer bounds)."""
    kf_side = matcher in ("fuse", "sim3_projection", "sim3_fuse", "by_sim3")
    g = O.Grid(s["k"], *s["bounds"], keyframe=kf_side)
    ur = _ur(s, matcher, p)
    if matcher == "last":
        return O.search_by_projection_last(g, ur, s["d"], s["sf"], CAM, s["T_cur"], s["T_last"], s["pos"], s["desc"], s["valid"], s["obs"],
                                           s["octave"], s["angle"], s["has"], p[0], p[1], p[2])
    if matcher == "points":
        return O.search_by_projection_points(g, ur, s["d"], s["sf"], oracle_frustum(s), s["desc"], s["obs"], s["has"], p[0], p[1])
    if matcher == "kf":
        return O.search_by_projection_kf(g, s["d"], s["sf"], CAM, s["T_cur"], LOG_SF, NL, s["pos"], s["desc"], s["valid"], s["angle"], s["max_d"],
                                         s["min_d"], s["has"], p[0], p[1], p[2])
    if matcher == "fuse":
        return O.fuse(g, ur, s["d"], s["sf"], s["inv_sigma2"], CAM, s["T_cur"], LOG_SF, NL, s["pos"], s["normal"], s["max_d"], s["min_d"], s["desc"],
                      s["valid"], p[0])
    if matcher in ("sim3_projection", "sim3_fuse"):
        mode = 0 if matcher == "sim3_projection" else 1
        return O.sim3_projection(mode, g, s["d"], s["sf"], CAM, s["Scw"], LOG_SF, NL, s["pos"], s["normal"], s["max_d"], s["min_d"], s["desc"], s["valid"],
                                 s["kf_matched"] if mode == 0 else None, p[0])
    g1 = O.Grid(s["k1"], *s["bounds"], keyframe=True)
    return O.search_by_sim3(g1, s["d1"], s["T_last"], s["pts1"], g, s["d"], s["T_cur"], s["pts2"], s["sf"], CAM, LOG_SF, NL, s["s12"], s["R12"], s["t12"], p[0])


def _obs_list(has):
    return [1 if h else None for h in has]  # the keypoint holds a point with Observations() == 1, or NULL


def literal_frustum(s, F, census=None):
    """Frame::isInFrustum of every valid point through the literal transcription: (points for search_by_projection_points, records)."""
    points, tp = [], np.zeros(len(s["pos"]), O.TP_DTYPE)
    for i in range(len(s["pos"])):
        t = LM.is_in_frustum(F, s["pos"][i], s["normal"][i], s["max_d"][i], s["min_d"][i], 0.5, LOG_SF, census)
        if t is None:
            points.append(None)
            continue
        tp[i] = (1, t["proj_x"], t["proj_y"], t["proj_xr"], t["level"], t["view_cos"])
        t["desc"] = s["desc"][i]; t["obs"] = int(s["obs"][i])
        points.append(t)
    return points, tp


def literal_run(matcher, s, p, census=None, frame_cls=LM.Frame, kf_cls=LK.KeyFrame):
    """(matches, count) of the literal transcription; census: a dict that receives the counters; frame_cls / kf_cls: the grid classes
    (the reference's, or a variant with a wrong window order)."""
    ur = _ur(s, matcher, p)
    F = frame_cls(s["k"], s["d"], ur, s["bounds"], CAMT, s["sf"], s["T_cur"])
    if matcher == "last":
        last = dict(pos=s["pos"], desc=s["desc"], valid=s["valid"], obs=s["obs"], octave=s["octave"], angle=s["angle"])
        return LM.search_by_projection_last(F, s["T_last"], last, _obs_list(s["has"]), p[0], p[1], p[2], census)
    if matcher == "points":
        points, _ = literal_frustum(s, F, census)
        return LM.search_by_projection_points(F, points, _obs_list(s["has"]), p[0], p[1], census)
    if matcher == "kf":
        kf = dict(pos=s["pos"], desc=s["desc"], valid=s["valid"], angle=s["angle"], max_distance=s["max_d"], min_distance=s["min_d"])
        return LM.search_by_projection_kf(F, kf, s["has"], p[0], p[1], p[2], LOG_SF, census)
    kf = kf_cls(F, s["inv_sigma2"], LOG_SF)
    points = dict(pos=s["pos"], normal=s["normal"], max_distance=s["max_d"], min_distance=s["min_d"], desc=s["desc"], valid=s["valid"])
    if matcher == "fuse":
        return LK.fuse(kf, s["T_cur"], points, p[0], census)
    if matcher == "sim3_projection":
        return LK.search_by_projection_sim3(kf, s["Scw"], points, s["kf_matched"], p[0], census)
    if matcher == "sim3_fuse":
        return LK.fuse_sim3(kf, s["Scw"], points, p[0], census)
    kf1 = kf_cls(frame_cls(s["k1"], s["d1"], None, s["bounds"], CAMT, s["sf"]), s["inv_sigma2"], LOG_SF)
    as_dict = lambda t: dict(pos=t[0], max_distance=t[1], min_distance=t[2], desc=t[3], valid=t[4])
    return LK.search_by_sim3(kf1, s["T_last"], as_dict(s["pts1"]), kf, s["T_cur"], as_dict(s["pts2"]), s["s12"], s["R12"], s["t12"], p[0], census)


def window_sizes(matcher, s, p):
    """Candidates per window as the ORACLE's grid counts them, for the windows the reference opens (from the literal run), and the
    number of queries the HIP entry point issues (one per map point row)."""
    census = {}
    literal_run(matcher, s, p, census)
    g = O.Grid(s["k"], *s["bounds"], keyframe=matcher in ("fuse", "sim3_projection", "sim3_fuse"))
    sizes = [len(g.features_in_area(x, y, r, lo, hi)) for x, y, r, lo, hi in census.get("_windows", [])]
    return sizes, len(s["pos"])


# every counter of the literal transcriptions; a function that has no such decision leaves it at 0
KEYS = ("invalid", "z_negative", "z_zero", "z_below_half", "z_negative_not_tested", "z_negative_in_image", "out_left", "out_right", "out_top",
        "out_bottom", "too_near", "too_far", "view_cos", "in_view", "level_clamped_low", "level_clamped_high", "radius_small", "radius_large",
        "window_outside_grid", "window_clipped_left", "window_clipped_right", "window_clipped_top", "window_clipped_bottom", "window_empty",
        "window_min_shared", "cand_below_level", "cand_above_level", "cand_uright_gate", "cand_chi2_stereo", "cand_chi2_mono",
        "cand_matched_on_entry", "cand_taken_in_call", "no_candidate_left", "best_above_threshold", "ratio_rejected", "ratio_other_level",
        "double_count", "rot_rejected", "motion_forward", "motion_backward", "motion_neither", "sim3_mutual", "sim3_one_direction_only",
        "sim3_mutual_disagree", "accepted", "accepted_on_tie", "tie_one_cell", "tie_one_column", "tie_columns_lower_index_later",
        "tie_columns_other", "tie_winner_not_lowest_index")


def counters(census):
    unknown = [k for k in census if not k.startswith("_") and k not in KEYS]
    assert not unknown, unknown
    return {k: int(census.get(k, 0)) for k in KEYS}


def census_of(name, matcher):
    """(oracle result, literal result, counters) of one census case."""
    s, p = build(name), INPUTS[name][1][matcher]
    census = {}
    lit = literal_run(matcher, s, p, census)
    return oracle_run(matcher, s, p), lit, counters(census)


if __name__ == "__main__":  # python -m tests.matcher_census: rewrite the pinned table after a deliberate change of an input
    import json
    import os
    table = {"%s/%s" % (name, m): census_of(name, m)[2] for name, m in CASES}
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN), "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
