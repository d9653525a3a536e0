"""Seeded problems for orbfe_enqueue_reconstruct_initial and its model (tests/reconstruct_model.py), built on tests/initializer_scenes.py:
the RANSAC winners come from the committed model of the call before (tests/initializer_model.py), so a problem here is the state that
orbfe_enqueue_find_homography_fundamental leaves in HBM plus K, sigma, min_triangulated and the model override.  Also the problem file
of tests/reconstruct_mirror/mirror_main.cpp."""
import functools
import struct

import numpy as np

from tests import initializer_scenes as S
from tests import reconstruct_model as R

F32 = np.float32
K4 = np.array([S.FX, S.FY, S.CX, S.CY], F32)
SENT_F32, SENT_I32, SENT_U8 = S.SENT_F32, S.SENT_I32, S.SENT_U8


def two_views(n_matches, iterations, rng, depth, Rm, t, noise=0.5, outliers=0.2, extra=None):
    """Two views as initializer_scenes.scene() draws them, of points at depth(ray) along the first camera's rays, moved by (Rm, t)."""
    W, H, FX, FY, CX, CY = S.WIDTH, S.HEIGHT, S.FX, S.FY, S.CX, S.CY
    extra1, extra2 = extra if extra is not None else (40 + n_matches // 10, 75 + n_matches // 8)
    pts1, pts2 = [], []
    while len(pts1) < n_matches:
        uv = rng.uniform([20, 20], [W - 20, H - 20])
        ray = np.array([(uv[0] - CX) / FX, (uv[1] - CY) / FY, 1.0])
        P = Rm @ (ray * depth(ray, rng)) + t
        uv2 = np.array([FX * P[0] / P[2] + CX, FY * P[1] / P[2] + CY])
        if P[2] > 0.5 and 20 <= uv2[0] < W - 20 and 20 <= uv2[1] < H - 20:
            pts1.append(uv); pts2.append(uv2)
    pts1, pts2 = np.array(pts1) + rng.normal(0, noise, (n_matches, 2)), np.array(pts2) + rng.normal(0, noise, (n_matches, 2))
    outlier = rng.random(n_matches) < outliers
    pts2[outlier] = rng.uniform([20, 20], [W - 20, H - 20], (int(outlier.sum()), 2))
    xy1 = np.concatenate([pts1, rng.uniform([20, 20], [W - 20, H - 20], (extra1, 2))])
    xy2 = np.concatenate([pts2, rng.uniform([20, 20], [W - 20, H - 20], (extra2, 2))])
    o1, o2 = rng.permutation(len(xy1)), rng.permutation(len(xy2))
    pos2 = np.empty(len(xy2), np.int64); pos2[o2] = np.arange(len(xy2))
    matches12 = np.where(o1 < n_matches, pos2[np.minimum(o1, n_matches - 1)], -1).astype(np.int32)
    p = S.problem(S.keys_of(xy1[o1].astype(F32)), S.keys_of(xy2[o2].astype(F32)), matches12, S.draw_sets(n_matches, iterations, rng))
    assert len(p["pairs"]) == n_matches
    return p


@functools.lru_cache(maxsize=None)
def ransac(kind, n_matches=300, iterations=200):
    """(problem, the RANSAC model's answer) of a named scene."""
    if kind in S.KINDS:
        return S.solved_scene(kind, n_matches, iterations)
    rng = np.random.default_rng([1, 2 + ("frontal", "sideways", "behind", "still").index(kind), n_matches])
    if kind == "frontal":       # a frontal plane at z = 4 seen from a sideways baseline of half its depth: the H ambiguity resolves
        p = two_views(n_matches, iterations, rng, lambda ray, g: 4.0, S._rot(0.02, 0.25, 0.01), np.array([-2.0, 0.1, 0.1]))
    elif kind == "sideways":    # noise-free pure sideways translation over general depth: the known answer
        p = two_views(n_matches, iterations, rng, lambda ray, g: g.uniform(2.0, 9.0), np.eye(3), np.array([-0.5, 0.0, 0.0]), noise=0.0, outliers=0.0)
    elif kind == "behind":      # the second view turned by 0.4 rad about the optical axis of a frontal plane under a small baseline
        p = two_views(n_matches, iterations, rng, lambda ray, g: 4.0, S._rot(0.0, 0.0, 0.4), np.array([-0.05, 0.0, 0.0]))
    else:                       # "still": a baseline of a millimetre: every point is counted, none has parallax (code 6)
        p = two_views(n_matches, iterations, rng, lambda ray, g: g.uniform(2.0, 9.0), S._rot(0.0, 0.0, 0.0), np.array([-0.001, 0.0, 0.0]), noise=0.05,
                      outliers=0.1)
    return p, S.solve(p)


def from_ransac(p, res, min_triangulated=50, model=-1, sigma=None):
    """The arguments of the call from a RANSAC problem and its answer (H21 / F21 untouched by RANSAC hold zeros)."""
    z = np.zeros(9, F32)
    return dict(keys1=p["keys1"], keys2=p["keys2"], pairs=p["pairs"].copy(), H21=(res["H21"] if res["H21"] is not None else z).astype(F32).copy(),
                F21=(res["F21"] if res["F21"] is not None else z).astype(F32).copy(), score=res["score"].astype(F32).copy(), best=res["best"].astype(np.int32).copy(),
                inl_h=res["inliers"][0].astype(np.uint8).copy(), inl_f=res["inliers"][1].astype(np.uint8).copy(), K=K4.copy(),
                sigma=F32(p["sigma"] if sigma is None else sigma), min_triangulated=int(min_triangulated), model=int(model), matches12=p["matches12"])


@functools.lru_cache(maxsize=None)
def scene(kind, n_matches=300, iterations=200, min_triangulated=50, model=-1):
    return from_ransac(*ransac(kind, n_matches, iterations), min_triangulated=min_triangulated, model=model)


def fresh(q, **changes):
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in q.items()}
    out.update(changes)
    return out


def identical_frames(model=0):
    p = S.identical_frames()
    return from_ransac(p, S.solve(p), model=model)


def with_flags(q, count, model):
    """The scene with only the first `count` of the model's set inlier flags kept (count 0: all flags zero)."""
    key = "inl_h" if model == 0 else "inl_f"
    f = q[key].copy()
    f[np.nonzero(f)[0][count:]] = 0
    return fresh(q, model=model, **{key: f})


_solved = {}


def solve(q, key=None):
    if key is not None and key in _solved:
        return _solved[key]
    out = R.reconstruct(q["keys1"], q["keys2"], q["pairs"], q["H21"], q["F21"], q["score"], q["best"], q["inl_h"], q["inl_f"], q["K"], q["sigma"],
                        q["min_triangulated"], q["model"])
    if key is not None:
        _solved[key] = out
    return out


def solved_scene(kind, n_matches=300, iterations=200, min_triangulated=50, model=-1):
    q = scene(kind, n_matches, iterations, min_triangulated, model)
    return q, solve(q, (kind, n_matches, iterations, min_triangulated, model))


class Outputs:
    """The outputs of one call, starting out as sentinels, and what the model expects in them."""
    NAMES = ("model", "hyp_R", "hyp_t", "ngood", "cos_parallax", "result", "choice", "R21", "t21", "p3d", "triangulated", "codes", "status")

    def __init__(self, q):
        n1, N = len(q["keys1"]), len(q["pairs"])
        self.model, self.result, self.choice, self.status = [np.full(1, SENT_I32, np.int32) for _ in range(4)]
        self.hyp_R, self.hyp_t = np.full((8, 9), SENT_F32, F32), np.full((8, 3), SENT_F32, F32)
        self.ngood, self.cos_parallax = np.full(8, SENT_I32, np.int32), np.full(8, SENT_F32, F32)
        self.R21, self.t21 = np.full(9, SENT_F32, F32), np.full(3, SENT_F32, F32)
        self.p3d, self.triangulated = np.full((n1, 3), SENT_F32, F32), np.full(n1, SENT_U8, np.uint8)
        self.codes = np.full((8, N), SENT_U8, np.uint8)

    @classmethod
    def expected(cls, q, res):
        o = cls(q)
        o.model[0], o.result[0], o.choice[0], o.status[0] = res["model"], res["result"], res["choice"], res["status"]
        o.hyp_R[:res["nhyp"]], o.hyp_t[:res["nhyp"]] = res["hyp_R"][:res["nhyp"]], res["hyp_t"][:res["nhyp"]]
        o.ngood[:], o.cos_parallax[:] = res["ngood"], res["cos_parallax"]
        if res["R21"] is not None:
            o.R21[:], o.t21[:] = res["R21"], res["t21"]
        o.p3d[:], o.triangulated[:], o.codes[:] = res["p3d"], res["triangulated"], res["codes"]
        return o


# ------------------------------------------------------------------ the mirror program's files
def write_problem_file(q, path):
    """int32 n1, n2, N, min_triangulated, model; float sigma, K[4], H21[9], F21[9], score[2]; int32 best[2]; x1[n1] y1[n1] x2[n2] y2[n2]
    (f32); pairs[2 N] (i32); inl_h[N] inl_f[N] (u8)"""
    with open(path, "wb") as f:
        f.write(struct.pack("<5i", len(q["keys1"]), len(q["keys2"]), len(q["pairs"]), q["min_triangulated"], q["model"]))
        f.write(struct.pack("<f", float(q["sigma"])))
        f.write(np.concatenate([q["K"], q["H21"], q["F21"], q["score"]]).astype(F32).tobytes())
        f.write(np.asarray(q["best"], np.int32).tobytes())
        for k in (q["keys1"], q["keys2"]):
            f.write(np.ascontiguousarray(k["x"], F32).tobytes()); f.write(np.ascontiguousarray(k["y"], F32).tobytes())
        f.write(np.ascontiguousarray(q["pairs"], np.int32).tobytes())
        f.write(np.ascontiguousarray(q["inl_h"], np.uint8).tobytes()); f.write(np.ascontiguousarray(q["inl_f"], np.uint8).tobytes())


def read_result_file(q, path):
    """int32 rc; then the outputs in Outputs.NAMES order without the status (status = rc)"""
    raw = open(path, "rb").read()
    o = Outputs(q)
    off = 4
    for name in Outputs.NAMES[:-1]:
        a = getattr(o, name)
        a[...] = np.frombuffer(raw, a.dtype, a.size, off).reshape(a.shape); off += a.nbytes
    assert off == len(raw)
    o.status[0] = struct.unpack_from("<i", raw, 0)[0]
    return o
