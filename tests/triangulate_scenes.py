"""Scenes for the triangulation stage of LocalMapping::CreateNewMapPoints (tests/triangulate_model.py), fixed by their seeds, the census
of what they decide, and the scene file of the C++ mirror (tests/triangulate_mirror/mirror_main.cpp).  No test here; everything is
computed once and cached -- callers copy what they change (fresh()).

two_view(name)   the two-view generator of tests/triangulation_scenes.py restated without a vocabulary: 1400 points (250 of them 60 to
                 400 m away: low parallax) seen from two poses with 0.4 px noise; half of the keypoints stereo (bf = 40, so mb = 0.08 m);
                 random octaves (the scale gate); every fifth pair deliberately wrong (reprojection and depth-sign failures).
                 "wide": the poses 0.4 m apart, every stereo pair is triangulated.  "narrow": 0.03 m apart, less than the stereo
                 baseline, so stereo keypoints are unprojected (codes 1 and 2) and monocular pairs have low parallax (code 3).
degenerate()     two cameras 2 m apart along x, both looking along z.  Pairs with x1 == x2 and y1 != y2 are skew rays whose fourth
                 column of A is exactly orthogonal to the others: w == 0 exactly (code 4).  Six copies of one true pair triangulate to
                 one point, and that point is handed over as KF2's Ow: distance zero (code 9).  Both hinge on exact float equalities, so
                 this scene has no float64 counterpart and is left out of the comparison with pair_f64().
"""
import numpy as np

from orbslam2_amd.api import KP_DTYPE
from tests import triangulate_model as M

F32, F64 = np.float32, np.float64
FX = FY = 500.0
CX, CY = 320.0, 240.0
MBF = F32(200.0)
NLEVELS = 8
N_KP = 1400
GENERIC = ("wide", "narrow", "forward")
# name -> (KF2's translation, its yaw in degrees, depth of the farthest near point, pairs)
VIEWS = {"wide": ((-1.5, 0.02, 0.05), 3.0, 30.0, 700), "narrow": ((-0.05, 0.003, 0.006), 0.3, 18.0, 500), "forward": ((0.0, 0.0, -12.0), 0.0, 18.0, 90)}
_CACHE = {}


def levels():
    """mvScaleFactor / mvLevelSigma2 of the default pyramid (8 levels, 1.2) by ORBextractor's own float recurrence."""
    sf = [F32(1)]
    for _ in range(1, NLEVELS):
        sf.append(F32(sf[-1] * F32(1.2)))
    return np.array(sf, F32), np.array([F32(s * s) for s in sf], F32)


RATIO_FACTOR = F32(F32(1.5) * levels()[0][1])


def _yaw(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def keyframe(T, n):
    """An empty keyframe of n keypoints under the double pose T (3x4): Tcw and Ow as float, the camera of the tests."""
    k = np.zeros(n, KP_DTYPE)
    k["size"] = 31; k["class_id"] = -1
    Tf = np.ascontiguousarray(T, F32).reshape(-1)
    Ow = np.ascontiguousarray(-T[:, :3].T @ T[:, 3], F32)
    kf = dict(keys_un=k, keys=k, ur=np.full(n, -1, F32), depth=np.full(n, -1, F32), cos=np.zeros(n, F32), mp=np.zeros(n, np.uint8), n=n,
              Tcw=Tf, Ow=Ow, fx=F32(FX), fy=F32(FY), cx=F32(CX), cy=F32(CY), invfx=F32(1.0 / FX), invfy=F32(1.0 / FY))
    return kf


def set_stereo(kf, i, u_right):
    """mvuRight, mvDepth = mbf / disparity (Frame::ComputeStereoMatches) and the caller's cos(2 atan2(mb / 2, depth))."""
    kf["ur"][i] = u_right
    kf["depth"][i] = MBF / F32(kf["keys_un"]["x"][i] - kf["ur"][i])
    mb = float(MBF) / FX
    kf["cos"][i] = np.cos(2 * np.arctan2(mb / 2, float(kf["depth"][i])))


def from_search_keyframe(kf, T, mbf=40.0):
    """A keyframe of tests/triangulation_scenes.py (bf = 40) as the model's dict: depth from the disparity, the caller's stereo cosine."""
    out = keyframe(T, len(kf["k"]))
    out["keys_un"] = out["keys"] = kf["k"].copy()
    out["ur"], out["mp"] = kf["ur"].copy(), kf["mp"].copy()
    st = out["ur"] >= 0
    out["depth"][st] = F32(mbf) / (out["keys_un"]["x"][st] - out["ur"][st])
    out["cos"][st] = np.cos(2 * np.arctan2(mbf / FX / 2, out["depth"][st].astype(F64)))
    return out


def _view(P, T, seen, seed):
    """Keypoint slot j sees point seen[j]."""
    r = np.random.default_rng(seed)
    n = len(seen)
    kf = keyframe(T, n)
    pc = (T[:, :3] @ P[seen].T).T + T[:, 3]
    k = kf["keys_un"]
    k["x"] = FX * pc[:, 0] / pc[:, 2] + CX + r.normal(0, 0.4, n)
    k["y"] = FY * pc[:, 1] / pc[:, 2] + CY + r.normal(0, 0.4, n)
    behind = pc[:, 2] < 0.5                         # not visible from here: the slot holds some other feature
    k["x"][behind] = r.uniform(20, 620, behind.sum()); k["y"][behind] = r.uniform(20, 460, behind.sum())
    k["octave"] = r.integers(0, NLEVELS, n)
    for i in np.nonzero((r.random(n) < 0.5) & (pc[:, 2] < 40) & ~behind)[0]:   # the stereo matcher finds no far point
        set_stereo(kf, i, F32(k["x"][i] - float(MBF) / pc[i, 2] + r.normal(0, 0.4)))
    bad = kf["ur"] >= k["x"]                       # no disparity left after the noise: a monocular keypoint
    kf["ur"][bad] = -1; kf["depth"][bad] = -1
    kf["mp"][:] = r.random(n) < 0.3
    return kf


def problem(kf1, kf2, pairs, max_pairs=None, npairs=None):
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1)
    count = len(pairs) // 2
    max_pairs = count if max_pairs is None else max_pairs
    buf = np.full(2 * max_pairs, -1, np.int32)
    buf[:len(pairs)] = pairs
    sf, s2 = levels()
    return dict(kf1=kf1, kf2=kf2, mbf=MBF, ratio=RATIO_FACTOR, pairs=buf, npairs=count if npairs is None else npairs, max_pairs=max_pairs, sf=sf, s2=s2)


def two_view(name, seed=5):
    if name not in _CACHE:
        t2, yaw, farthest, n_pairs = VIEWS[name]
        rng = np.random.default_rng(21)
        n = N_KP
        P = np.stack([rng.uniform(-6, 6, n), rng.uniform(-4, 4, n), rng.uniform(4, farthest, n)], axis=1)
        far = rng.choice(n, 250, replace=False)
        P[far] *= (rng.uniform(60, 400, 250) / P[far, 2])[:, None]
        T1 = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
        T2 = np.concatenate([_yaw(yaw), np.array(t2)[:, None]], axis=1)
        r = np.random.default_rng(seed)
        seen2 = r.permutation(n)
        slot2 = np.argsort(seen2)
        kf1, kf2 = _view(P, T1, np.arange(n), 1), _view(P, T2, seen2, 2)
        pool = np.arange(n)
        if name == "forward":                                       # near points only, found again at their KF1 pixel: parallel rays
            pool = np.nonzero(P[:, 2] < 19.0)[0]
            for c in ("x", "y"):
                kf2["keys_un"][c][slot2[pool]] = kf1["keys_un"][c][pool] + r.normal(0, 0.4, len(pool)).astype(F32)
        idx1 = np.sort(r.choice(pool, n_pairs, replace=False))      # ascending idx1, as SearchForTriangulation leaves them
        idx2 = slot2[idx1]
        wrong = np.nonzero(r.random(n_pairs) < 0.2)[0]
        free = np.setdiff1d(np.arange(n), idx2)
        idx2[wrong] = r.choice(free, len(wrong), replace=False)     # a KF2 keypoint is matched at most once
        _CACHE[name] = problem(kf1, kf2, np.stack([idx1, idx2], axis=1))
    return _CACHE[name]


def degenerate():
    if "degenerate" not in _CACHE:
        r = np.random.default_rng(8)
        T1 = np.concatenate([np.eye(3), np.array([[-1.0], [0.0], [0.0]])], axis=1)
        T2 = np.concatenate([np.eye(3), np.array([[1.0], [0.0], [0.0]])], axis=1)
        n_w0, n_dup, n = 8, 6, 20
        kf1, kf2 = keyframe(T1, n), keyframe(T2, n)
        for kf in (kf1, kf2):
            kf["keys_un"]["x"] = r.uniform(100, 540, n); kf["keys_un"]["y"] = r.uniform(100, 380, n); kf["keys_un"]["octave"] = 2
        pairs = []
        for q in range(n_w0):                                       # the same column in both images, rows 20 to 60 px apart
            i1, i2 = q, n - 1 - q
            kf2["keys_un"]["x"][i2] = kf1["keys_un"]["x"][i1]
            kf2["keys_un"]["y"][i2] = kf1["keys_un"]["y"][i1] + r.uniform(20, 60) * (1 if q % 2 else -1)
            pairs.append((i1, i2))
        Pw = np.array([0.3, -0.2, 9.0])
        for q in range(n_dup):
            i1, i2 = n_w0 + q, n - 1 - n_w0 - q
            for kf, T, i in ((kf1, T1, i1), (kf2, T2, i2)):
                pc = T[:, :3] @ Pw + T[:, 3]
                kf["keys_un"]["x"][i] = FX * pc[0] / pc[2] + CX; kf["keys_un"]["y"][i] = FY * pc[1] / pc[2] + CY
            pairs.append((i1, i2))
        sf, s2 = levels()
        c, X, _ = M.pair(kf1, kf2, n_w0, n - 1 - n_w0, MBF, RATIO_FACTOR, sf, s2)
        assert c == M.TRIANGULATED
        kf2["Ow"] = np.array(X, F32)                                # GetCameraCenter() is handed over, not recomputed
        _CACHE["degenerate"] = problem(kf1, kf2, pairs)
    return _CACHE["degenerate"]


def scene(name):
    return degenerate() if name == "degenerate" else two_view(name)


SCENES = GENERIC + ("degenerate",)


def fresh(p, **changes):
    """A deep copy of a problem (keyframes and arrays) with changes applied: the model, the mirror and the device all write has_mp."""
    q = dict(p)
    for kf in ("kf1", "kf2"):
        q[kf] = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p[kf].items()}
        if p[kf]["keys"] is p[kf]["keys_un"]:
            q[kf]["keys"] = q[kf]["keys_un"]
    q["pairs"] = p["pairs"].copy()
    q.update(changes)
    return q


def with_distorted_keys(p, seed=3):
    """mvKeys != mvKeysUn: a smooth radial displacement of up to a few pixels, read only by UnprojectStereo."""
    q = fresh(p)
    for kf in ("kf1", "kf2"):
        k = q[kf]["keys_un"].copy()
        dx, dy = k["x"] - F32(CX), k["y"] - F32(CY)
        r2 = (dx * dx + dy * dy) / F32(320.0 ** 2)
        k["x"] = k["x"] - dx * F32(0.02) * r2; k["y"] = k["y"] - dy * F32(0.02) * r2
        q[kf]["keys"] = k
    return q


class Outputs:
    """The output block of one call, filled with sentinels."""
    SENT_U8, SENT_I32 = 0xA5, -7

    def __init__(self, p, n_rows=None, rows_used=0):
        m = p["max_pairs"]
        self.code = np.full(m, self.SENT_U8, np.uint8)
        self.x3d = np.full((m, 3), np.float32(-777.0), F32)
        self.new = np.full(3 * m, self.SENT_I32, np.int32)
        self.n_rows, self.rows_used = n_rows, rows_used
        self.pos = None if n_rows is None else np.full((n_rows, 3), np.float32(-555.0), F32)


def run_model(p, out, patch=1):
    """The model on a problem (has_mp of p's keyframes is written) into `out`; returns its result dict."""
    return M.triangulate_pairs(p["kf1"], p["kf2"], p["mbf"], p["ratio"], p["pairs"], p["npairs"], p["max_pairs"], p["sf"], p["s2"], out.code, out.x3d,
                               out.new, pos=out.pos, n_rows=out.n_rows or 0, rows_used=out.rows_used, patch_has_mp=patch)


def census(name):
    """Per scene, once: (codes, x3d, infos, result) of the model without a table and without the patch."""
    key = ("census", name)
    if key not in _CACHE:
        p = fresh(scene(name))
        out = Outputs(p)
        res = run_model(p, out, patch=0)
        _CACHE[key] = (out.code.copy(), out.x3d.copy(), res["infos"], res)
    return _CACHE[key]


# ------------------------------------------------------------------ the mirror's files
def write_problem_file(p, out, patch, path):
    """int32 n1, n2, npairs, max_pairs, nlevels, has_pos, n_rows, rows_used, patch; float32 mbf, ratio; per keyframe Tcw[12] Ow[3] fx fy cx cy
    invfx invfy, then x_un y_un (f32) octave (i32) x y ur depth cos (f32) mp (u8); pairs; sf s2; code x3d new pos as the caller holds them."""
    with open(path, "wb") as f:
        has_pos = out.pos is not None
        np.array([p["kf1"]["n"], p["kf2"]["n"], p["npairs"], p["max_pairs"], len(p["sf"]), int(has_pos), out.n_rows or 0, out.rows_used, patch],
                 np.int32).tofile(f)
        np.array([p["mbf"], p["ratio"]], F32).tofile(f)
        for kf in (p["kf1"], p["kf2"]):
            np.concatenate([kf["Tcw"], kf["Ow"], [kf[k] for k in ("fx", "fy", "cx", "cy", "invfx", "invfy")]]).astype(F32).tofile(f)
            n = kf["n"]
            for a, t in ((kf["keys_un"]["x"], F32), (kf["keys_un"]["y"], F32), (kf["keys_un"]["octave"], np.int32), (kf["keys"]["x"], F32),
                         (kf["keys"]["y"], F32), (kf["ur"], F32), (kf["depth"], F32), (kf["cos"], F32), (kf["mp"], np.uint8)):
                np.ascontiguousarray(a[:n], t).tofile(f)
        p["pairs"].tofile(f); p["sf"].tofile(f); p["s2"].tofile(f)
        out.code.tofile(f); out.x3d.tofile(f); out.new.tofile(f)
        if has_pos:
            out.pos.tofile(f)


def read_result_file(p, out, path):
    """int32 status, nnew (-7: untouched), rows_used; code, x3d, new, pos, mp1, mp2.  Returns (result dict, Outputs, mp1, mp2)."""
    raw = np.fromfile(path, np.uint8)
    m, at = p["max_pairs"], [0]

    def take(count, dtype):
        nbytes = count * np.dtype(dtype).itemsize
        a = raw[at[0]: at[0] + nbytes].view(dtype).copy()
        at[0] += nbytes
        return a

    status, nnew, rows_used = take(3, np.int32).tolist()
    got = Outputs(p, out.n_rows, rows_used)
    got.code, got.x3d, got.new = take(m, np.uint8), take(3 * m, F32).reshape(m, 3), take(3 * m, np.int32)
    if out.pos is not None:
        got.pos = take(3 * out.n_rows, F32).reshape(-1, 3)
    mp1, mp2 = take(p["kf1"]["n"], np.uint8), take(p["kf2"]["n"], np.uint8)
    assert at[0] == len(raw)
    return dict(status=status, nnew=None if nnew == Outputs.SENT_I32 else nnew, rows_used=rows_used), got, mp1, mp2
