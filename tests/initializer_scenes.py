"""Seeded problems for orbfe_enqueue_find_homography_fundamental and its model (tests/initializer_model.py): two views of a general-depth or
a planar scene at the Tracking geometry (640 x 480, f = 520), 0.5 px noise, 20 % outliers, the sets drawn as Initializer::Initialize draws
them (:81-96, with a seeded numpy generator in place of rand()).  The two frames hold different numbers of keypoints in shuffled order, so
vMatches12 has -1 entries and mvMatches12 is not the identity.  Also the problem file of tests/initializer_mirror/mirror_main.cpp."""
import functools
import struct

import numpy as np

from tests import initializer_model as M

F32 = np.float32
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
FX = FY = 520.0
CX, CY, WIDTH, HEIGHT = 320.0, 240.0, 640, 480
KINDS = ("general", "planar")
SENT_F32, SENT_I32, SENT_U8 = F32(-555.0), -7, 0xEE


def keys_of(xy):
    k = np.zeros(len(xy), KP_DTYPE)
    k["x"], k["y"], k["size"], k["angle"] = xy[:, 0], xy[:, 1], 31.0, -1.0
    return k


def draw_sets(n_matches, iterations, rng):
    """mvSets (:81-96): eight distinct matches per iteration, drawn by swapping the chosen index with the last available one."""
    sets = np.zeros((iterations, 8), np.int32)
    for it in range(iterations):
        avail = list(range(n_matches))
        for j in range(8):
            r = int(rng.integers(0, len(avail)))
            sets[it, j] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return sets


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def problem(keys1, keys2, matches12, sets, sigma=1.0):
    """The arguments of the call from two keypoint arrays and vMatches12: mvMatches12 compacted (:50-62), Normalize of both frames."""
    matches12 = np.asarray(matches12, np.int32)
    i = np.nonzero(matches12 >= 0)[0]
    pairs = np.stack([i, matches12[i]], axis=1).astype(np.int32)
    return dict(keys1=keys1, keys2=keys2, matches12=matches12, pairs=pairs, sets=np.asarray(sets, np.int32).reshape(-1, 8), norm1=M.normalize_keys(keys1),
                norm2=M.normalize_keys(keys2), sigma=F32(sigma))


@functools.lru_cache(maxsize=None)
def scene(kind, n_matches=300, iterations=200, seed=1):
    rng = np.random.default_rng([seed, KINDS.index(kind), n_matches])
    extra1, extra2 = 40 + n_matches // 10, 75 + n_matches // 8          # n1 != n2
    R, t = _rot(0.03, -0.05, 0.02), np.array([-0.35, 0.06, 0.04])
    pts1, pts2 = [], []
    while len(pts1) < n_matches:
        uv = rng.uniform([20, 20], [WIDTH - 20, HEIGHT - 20])
        ray = np.array([(uv[0] - CX) / FX, (uv[1] - CY) / FY, 1.0])
        z = rng.uniform(2.0, 9.0) if kind == "general" else 5.0 / (1.0 + 0.25 * ray[0] - 0.15 * ray[1])    # the plane 0.25 x - 0.15 y + z = 5
        P = R @ (ray * z) + t
        uv2 = np.array([FX * P[0] / P[2] + CX, FY * P[1] / P[2] + CY])
        if P[2] > 0.5 and 20 <= uv2[0] < WIDTH - 20 and 20 <= uv2[1] < HEIGHT - 20:
            pts1.append(uv); pts2.append(uv2)
    pts1, pts2 = np.array(pts1) + rng.normal(0, 0.5, (n_matches, 2)), np.array(pts2) + rng.normal(0, 0.5, (n_matches, 2))
    outlier = rng.random(n_matches) < 0.2
    pts2[outlier] = rng.uniform([20, 20], [WIDTH - 20, HEIGHT - 20], (int(outlier.sum()), 2))
    xy1 = np.concatenate([pts1, rng.uniform([20, 20], [WIDTH - 20, HEIGHT - 20], (extra1, 2))])
    xy2 = np.concatenate([pts2, rng.uniform([20, 20], [WIDTH - 20, HEIGHT - 20], (extra2, 2))])
    o1, o2 = rng.permutation(len(xy1)), rng.permutation(len(xy2))          # new index -> old index
    pos2 = np.empty(len(xy2), np.int64); pos2[o2] = np.arange(len(xy2))
    matches12 = np.where(o1 < n_matches, pos2[np.minimum(o1, n_matches - 1)], -1).astype(np.int32)
    p = problem(keys_of(xy1[o1].astype(F32)), keys_of(xy2[o2].astype(F32)), matches12, draw_sets(n_matches, iterations, rng))
    assert len(p["pairs"]) == n_matches
    p["outlier"] = outlier[o1[p["pairs"][:, 0]]]
    return p


def fresh(p, **changes):
    q = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    q.update(changes)
    return q


def with_sets(p, sets):
    return fresh(p, sets=np.asarray(sets, np.int32).reshape(-1, 8))


def identical_frames(n=40, iterations=12, seed=5):
    """Both frames are the same keypoints, matched one to one: H = I exactly fits every match."""
    rng = np.random.default_rng(seed)
    keys = keys_of(rng.uniform([20, 20], [WIDTH - 20, HEIGHT - 20], (n, 2)).astype(F32))
    return problem(keys, keys.copy(), np.arange(n), draw_sets(n, iterations, rng))


def unrelated_frames(n=40, iterations=12, seed=6, sigma=1e-4):
    """Matches between unrelated points under a sigma of a ten-thousandth of a pixel: no hypothesis brings any match under its threshold."""
    rng = np.random.default_rng(seed)
    k1 = keys_of(rng.uniform([20, 20], [WIDTH - 20, HEIGHT - 20], (n, 2)).astype(F32))
    k2 = keys_of(rng.uniform([20, 20], [WIDTH - 20, HEIGHT - 20], (n + 3, 2)).astype(F32))
    return problem(k1, k2, rng.permutation(n + 3)[:n], draw_sets(n, iterations, rng), sigma=sigma)


_solved = {}


def solve(p, key=None):
    """The model's answer; cached under `key`."""
    if key is not None and key in _solved:
        return _solved[key]
    out = M.find(p["keys1"], p["keys2"], p["pairs"], p["sets"], p["norm1"], p["norm2"], p["sigma"])
    if key is not None:
        _solved[key] = out
    return out


def solved_scene(kind, n_matches=300, iterations=200, seed=1):
    p = scene(kind, n_matches, iterations, seed)
    return p, solve(p, (kind, n_matches, iterations, seed))


class Outputs:
    """The outputs of one call, starting out as sentinels, and what the model expects in them."""

    def __init__(self, p):
        N, B = len(p["pairs"]), len(p["sets"])
        self.H21, self.F21 = np.full(9, SENT_F32, F32), np.full(9, SENT_F32, F32)
        self.score, self.best = np.full(2, SENT_F32, F32), np.full(2, SENT_I32, np.int32)
        self.inl_h, self.inl_f = np.full(N, SENT_U8, np.uint8), np.full(N, SENT_U8, np.uint8)
        self.ninliers, self.all_scores = np.full(2, SENT_I32, np.int32), np.full((2, B), SENT_F32, F32)
        self.status = np.full(1, SENT_I32, np.int32)

    NAMES = ("H21", "F21", "score", "best", "inl_h", "inl_f", "ninliers", "all_scores", "status")

    @classmethod
    def expected(cls, p, res):
        o = cls(p)
        if res["H21"] is not None:
            o.H21[:] = res["H21"]
        if res["F21"] is not None:
            o.F21[:] = res["F21"]
        o.score[:], o.best[:], o.ninliers[:] = res["score"], res["best"], res["ninliers"]
        o.inl_h[:], o.inl_f[:] = res["inliers"][0], res["inliers"][1]
        o.all_scores[:] = res["all_scores"]
        o.status[0] = res["status"]
        return o


# ------------------------------------------------------------------ the mirror program's files
def write_problem_file(p, path):
    """int32 n1, n2, N, iterations, norms_given; float sigma, norm1[4], norm2[4] (used when norms_given, else the program's own Normalize);
    x1[n1] y1[n1] x2[n2] y2[n2] (f32); pairs[2 N] sets[8 iterations] (i32)"""
    with open(path, "wb") as f:
        f.write(struct.pack("<5i", len(p["keys1"]), len(p["keys2"]), len(p["pairs"]), len(p["sets"]), int(bool(p.get("norms_given")))))
        f.write(struct.pack("<f", float(p["sigma"])))
        f.write(np.concatenate([p["norm1"], p["norm2"]]).astype(F32).tobytes())
        for k in (p["keys1"], p["keys2"]):
            f.write(np.ascontiguousarray(k["x"], F32).tobytes()); f.write(np.ascontiguousarray(k["y"], F32).tobytes())
        f.write(np.ascontiguousarray(p["pairs"], np.int32).tobytes()); f.write(np.ascontiguousarray(p["sets"], np.int32).tobytes())


def read_result_file(p, path):
    """int32 rc; norm1[4] norm2[4] (the program's own Normalize); then the outputs in Outputs.NAMES order (status = rc)"""
    raw = open(path, "rb").read()
    o = Outputs(p)
    rc = struct.unpack_from("<i", raw, 0)[0]
    off = 4
    norms = np.frombuffer(raw, F32, 8, off).copy(); off += 32
    for name in Outputs.NAMES[:-1]:
        a = getattr(o, name)
        a[...] = np.frombuffer(raw, a.dtype, a.size, off).reshape(a.shape); off += a.nbytes
    assert off == len(raw)
    o.status[0] = rc
    return norms[:4], norms[4:], o
