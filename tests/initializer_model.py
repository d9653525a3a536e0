"""Literal model of Initializer::FindHomography and Initializer::FindFundamental (reference src/Initializer.cc:123-467, with Normalize,
:748-794) on the flat arrays of orbfe_enqueue_find_homography_fundamental (include/orbfe.h).  Every float step is an explicit np.float32 /
np.float64 operation in the reference's order; numpy arrays run ACROSS the independent hypotheses only (axis 0), never along a sum: the
double dot products, the square sums and the score are Python loops in index / match order.  It is the reference of
tests/test_initializer_model.py (against orbslam2_amd/host/Initializer.h) and tests/test_initializer_device.py (against the kernels); both
must equal it bit for bit.  find_f64() is the same pipeline in double with numpy.linalg.svd and numpy.linalg.inv.

Float contract (Q4: no contraction, IEEE divide and sqrt; the OpenCV steps are OPENCV-4.5.5-SEMANTICS, unpinned, stated in DESIGN.md
sections 4i2 and 4l; the cv::Mat rules themselves are tests/cvmat_model.py's):
  normalised point          ((x - meanX) * sX, (y - meanY) * sY) in float
  rows of A                 the float products of :238-256 / :280-288; F's 8 x 9 matrix gets a zero ninth row
  cv::SVDecomp -> vt.row(8) jacobi() on 9 columns (m = 16 / 9 rows); OpenCV's own m < n path is not restated
  rank-2 step               svd3() of the 3 x 3 Fpre, w[2] = 0, (u * diag(w)) * vt
  Mat * Mat, Mat::inv       mat(), inv3()
  CheckHomography / CheckFundamental   float, left to right; 1.0 / x in double, rounded; NaN > th is false, so NaN joins the score
  score                     sequential float sum in match order; the winner is the first strict maximum above 0
"""
import numpy as np

from tests.cvmat_model import AS, F32, F64, MAX_SWEEPS, NAN_BITS, inv3, jacobi, mat, stored, svd3  # noqa: F401 (constants read through this module)

ERR_INVALID = -1
TH_H = F32(5.991)
TH_F, TH_SCORE_F = F32(3.841), F32(5.991)
MAX_MATCHES, MAX_ITERATIONS, MAX_KEYS = 65535, 65535, 1 << 24


# ------------------------------------------------------------------ Normalize
def normalize_keys(keys):
    """Initializer::Normalize (:748-794): (meanX, meanY, sX, sY) as float32[4]; sequential float sums in keypoint order."""
    n = len(keys)
    with np.errstate(all="ignore"):
        mx, my = F32(0), F32(0)
        for i in range(n):
            mx = F32(mx + keys["x"][i]); my = F32(my + keys["y"][i])
        mx, my = F32(mx / F32(n)), F32(my / F32(n))
        dx, dy = F32(0), F32(0)
        for i in range(n):
            dx = F32(dx + abs(F32(keys["x"][i] - mx))); dy = F32(dy + abs(F32(keys["y"][i] - my)))
        dx, dy = F32(dx / F32(n)), F32(dy / F32(n))
        return np.array([mx, my, F32(F64(1.0) / F64(dx)), F32(F64(1.0) / F64(dy))], F32)


def t_matrix(norm):
    T = np.zeros((3, 3), F32)
    T[0, 0], T[1, 1], T[2, 2] = norm[2], norm[3], 1
    T[0, 2], T[1, 2] = F32(-norm[0] * norm[2]), F32(-norm[1] * norm[3])
    return T


# ------------------------------------------------------------------ the two 8-point solutions
def compute_h21(p1, p2):
    """ComputeH21 (:225-265) for B sets: p1, p2 float32[B][8][2] normalised points.  Returns (Hn float32[B][3][3], info)."""
    B = p1.shape[0]
    At = np.zeros((B, 9, AS), F32)
    zero, one = np.zeros(B, F32), np.ones(B, F32)
    for i in range(8):
        u1, v1, u2, v2 = p1[:, i, 0], p1[:, i, 1], p2[:, i, 0], p2[:, i, 1]
        r0 = [zero, zero, zero, -u1, -v1, -one, v2 * u1, v2 * v1, v2]
        r1 = [u1, v1, one, zero, zero, zero, (-u2) * u1, (-u2) * v1, -u2]
        for c in range(9):
            At[:, c, 2 * i], At[:, c, 2 * i + 1] = r0[c], r1[c]
    _, Vt, _, info = jacobi(At, 9, 16)
    return Vt[:, 8, :9].reshape(B, 3, 3).copy(), info


def compute_f21(p1, p2):
    """ComputeF21 (:267-302) for B sets.  Returns (Fn float32[B][3][3], info of the 9-column Jacobi, info of the 3 x 3 one)."""
    B = p1.shape[0]
    At = np.zeros((B, 9, AS), F32)
    one = np.ones(B, F32)
    for i in range(8):
        u1, v1, u2, v2 = p1[:, i, 0], p1[:, i, 1], p2[:, i, 0], p2[:, i, 1]
        r = [u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, one]
        for c in range(9):
            At[:, c, i] = r[c]
    _, Vt, _, info = jacobi(At, 9, 9)          # row 8 of A is zero
    u, w, vt, info3 = svd3(Vt[:, 8, :9].reshape(B, 3, 3))
    d = np.zeros((B, 3, 3), F32)
    d[:, 0, 0], d[:, 1, 1] = w[:, 0], w[:, 1]      # w.at<float>(2) = 0
    return mat(mat(u, d), vt), info, info3


# ------------------------------------------------------------------ the scores
def _chi_h(H21, H12, u1, v1, u2, v2, inv_sigma2):
    """The two chi-squares of one match under B homographies (H21, H12 float32[B][9]); u1 .. v2 float32 scalars."""
    w2 = (F64(1.0) / ((H12[:, 6] * u2 + H12[:, 7] * v2) + H12[:, 8]).astype(F64)).astype(F32)
    u2in1 = ((H12[:, 0] * u2 + H12[:, 1] * v2) + H12[:, 2]) * w2
    v2in1 = ((H12[:, 3] * u2 + H12[:, 4] * v2) + H12[:, 5]) * w2
    chi1 = ((u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1)) * inv_sigma2
    w1 = (F64(1.0) / ((H21[:, 6] * u1 + H21[:, 7] * v1) + H21[:, 8]).astype(F64)).astype(F32)
    u1in2 = ((H21[:, 0] * u1 + H21[:, 1] * v1) + H21[:, 2]) * w1
    v1in2 = ((H21[:, 3] * u1 + H21[:, 4] * v1) + H21[:, 5]) * w1
    chi2 = ((u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2)) * inv_sigma2
    assert chi1.dtype == F32 and chi2.dtype == F32
    return chi1, chi2


def _chi_f(F, u1, v1, u2, v2, inv_sigma2):
    a2 = (F[:, 0] * u1 + F[:, 1] * v1) + F[:, 2]
    b2 = (F[:, 3] * u1 + F[:, 4] * v1) + F[:, 5]
    c2 = (F[:, 6] * u1 + F[:, 7] * v1) + F[:, 8]
    num2 = (a2 * u2 + b2 * v2) + c2
    chi1 = ((num2 * num2) / (a2 * a2 + b2 * b2)) * inv_sigma2
    a1 = (F[:, 0] * u2 + F[:, 3] * v2) + F[:, 6]
    b1 = (F[:, 1] * u2 + F[:, 4] * v2) + F[:, 7]
    c1 = (F[:, 2] * u2 + F[:, 5] * v2) + F[:, 8]
    num1 = (a1 * u1 + b1 * v1) + c1
    chi2 = ((num1 * num1) / (a1 * a1 + b1 * b1)) * inv_sigma2
    assert chi1.dtype == F32 and chi2.dtype == F32
    return chi1, chi2


def check(model, mats, keys1, keys2, pairs, pair_ok, inv_sigma2):
    """CheckHomography (model 0, mats = (H21, H12)) / CheckFundamental (model 1, mats = (F21,)) of B hypotheses over all matches.
    Returns (score float32[B], inlier bool[B][N], added bool[B][N]: the match added a term)."""
    B, N = mats[0].shape[0], len(pairs)
    score = np.zeros(B, F32)
    inl, added = np.zeros((B, N), bool), np.zeros((B, N), bool)
    th, th_score = (TH_H, TH_H) if model == 0 else (TH_F, TH_SCORE_F)
    for i in range(N):
        if not pair_ok[i]:
            continue          # a faulty match adds nothing
        u1, v1 = F32(keys1["x"][pairs[i, 0]]), F32(keys1["y"][pairs[i, 0]])
        u2, v2 = F32(keys2["x"][pairs[i, 1]]), F32(keys2["y"][pairs[i, 1]])
        chi1, chi2 = _chi_h(mats[0], mats[1], u1, v1, u2, v2, inv_sigma2) if model == 0 else _chi_f(mats[0], u1, v1, u2, v2, inv_sigma2)
        out1, out2 = chi1 > th, chi2 > th           # false for NaN
        score = np.where(out1, score, score + (th_score - chi1))
        score = np.where(out2, score, score + (th_score - chi2))
        inl[:, i] = ~out1 & ~out2
        added[:, i] = ~out1 | ~out2
    assert score.dtype == F32
    return score, inl, added


def first_strict_maximum(scores):
    """`if (currentScore > score)` from score = 0 in iteration order (:164, :215).  Returns (iteration or -1, score)."""
    best, score = -1, scores.dtype.type(0)
    for it in range(len(scores)):
        if scores[it] > score:
            best, score = it, scores[it]
    return best, score


# ------------------------------------------------------------------ the call
def refused(n1, n2, N, iterations, sigma):
    return N < 8 or N > MAX_MATCHES or iterations < 1 or iterations > MAX_ITERATIONS or n1 < 0 or n2 < 0 or n1 > MAX_KEYS or n2 > MAX_KEYS or not sigma > 0


def find(keys1, keys2, pairs, sets, norm1, norm2, sigma):
    """orbfe_enqueue_find_homography_fundamental on numpy arrays: keys structured (x, y), pairs int32[N][2], sets int32[iterations][8],
    norm float32[4].  Returns dict(status, H21, F21 (float32[9] or None: untouched), score float32[2], best int32[2], inliers uint8[2][N],
    ninliers int32[2], all_scores float32[2][iterations] (as stored), ok bool[iterations], added / inliers_all bool[2][iterations][N] (every hypothesis's terms and flags), mats, infos)."""
    pairs, sets = np.asarray(pairs, np.int32).reshape(-1, 2), np.asarray(sets, np.int32).reshape(-1, 8)
    n1, n2, N, B = len(keys1), len(keys2), len(pairs), len(sets)
    assert not refused(n1, n2, N, B, sigma)
    norm1, norm2, sigma = np.asarray(norm1, F32), np.asarray(norm2, F32), F32(sigma)
    with np.errstate(all="ignore"):
        pair_ok = (pairs[:, 0] >= 0) & (pairs[:, 0] < n1) & (pairs[:, 1] >= 0) & (pairs[:, 1] < n2)
        set_ok = (sets >= 0) & (sets < N)
        ok = set_ok.all(axis=1) & pair_ok[np.where(set_ok, sets, 0)].all(axis=1)
        status = 0 if pair_ok.all() and ok.all() else ERR_INVALID
        T1, T2 = t_matrix(norm1), t_matrix(norm2)
        T2inv, T2t = inv3(T2), T2.T.copy()
        inv_sigma2 = F32(F64(1.0) / F64(F32(sigma * sigma)))
        # Select a minimum set (a faulty hypothesis computes on match 0's stand-in and is overruled below)
        idx = np.where(ok[:, None], sets, 0)
        i1 = np.clip(pairs[idx, 0], 0, max(n1 - 1, 0)); i2 = np.clip(pairs[idx, 1], 0, max(n2 - 1, 0))
        p1 = np.stack([(keys1["x"][i1].astype(F32) - norm1[0]) * norm1[2], (keys1["y"][i1].astype(F32) - norm1[1]) * norm1[3]], axis=-1)
        p2 = np.stack([(keys2["x"][i2].astype(F32) - norm2[0]) * norm2[2], (keys2["y"][i2].astype(F32) - norm2[1]) * norm2[3]], axis=-1)
        assert p1.dtype == F32
        Hn, info_h = compute_h21(p1, p2)
        H21 = mat(mat(T2inv, Hn), T1)
        H12 = inv3(H21)
        Fn, info_f, info_f3 = compute_f21(p1, p2)
        F21 = mat(mat(T2t, Fn), T1)
        mats = [(H21.reshape(B, 9), H12.reshape(B, 9)), (F21.reshape(B, 9),)]
        out = dict(status=status, ok=ok, mats=mats, infos=(info_h, info_f, info_f3), H21=None, F21=None, score=np.zeros(2, F32), best=np.zeros(2, np.int32),
                   inliers=np.zeros((2, N), np.uint8), ninliers=np.zeros(2, np.int32), all_scores=np.zeros((2, B), F32), added=np.zeros((2, B, N), bool), inliers_all=np.zeros((2, B, N), bool))
        for model in range(2):
            score, inl, added = check(model, mats[model], keys1, keys2, pairs, pair_ok, inv_sigma2)
            score = np.where(ok, score, F32(0)).astype(F32)       # a faulty hypothesis is skipped
            out["all_scores"][model] = stored(score)
            out["added"][model] = added & ok[:, None]
            out["inliers_all"][model] = inl & ok[:, None]
            best, s = first_strict_maximum(score)
            out["best"][model], out["score"][model] = best, s
            if best >= 0:
                out["H21" if model == 0 else "F21"] = mats[model][0][best].copy()
                out["inliers"][model] = inl[best]
                out["ninliers"][model] = int(inl[best].sum())
        return out


# ------------------------------------------------------------------ the float64 restatement
def find_f64(keys1, keys2, pairs, sets, norm1, norm2, sigma):
    """The same pipeline in double with numpy.linalg.svd / inv, for problems without faulty indices.  Returns dict(scores float64[2][B],
    best[2], score[2], chi float64[2][B][N][2], th (the two flag thresholds))."""
    pairs, sets = np.asarray(pairs, np.int64).reshape(-1, 2), np.asarray(sets, np.int64).reshape(-1, 8)
    B = len(sets)
    n1_, n2_ = np.asarray(norm1, F64), np.asarray(norm2, F64)

    def T(n):
        return np.array([[n[2], 0, -n[0] * n[2]], [0, n[3], -n[1] * n[3]], [0, 0, 1]], F64)

    x1 = np.stack([keys1["x"][pairs[:, 0]], keys1["y"][pairs[:, 0]]], axis=-1).astype(F64)
    x2 = np.stack([keys2["x"][pairs[:, 1]], keys2["y"][pairs[:, 1]]], axis=-1).astype(F64)
    T1, T2 = T(n1_), T(n2_)
    p1 = (x1[sets] - n1_[:2]) * n1_[2:]
    p2 = (x2[sets] - n2_[:2]) * n2_[2:]
    u1, v1, u2, v2 = p1[..., 0], p1[..., 1], p2[..., 0], p2[..., 1]
    z, o = np.zeros_like(u1), np.ones_like(u1)
    A = np.empty((B, 16, 9))
    A[:, 0::2] = np.stack([z, z, z, -u1, -v1, -o, v2 * u1, v2 * v1, v2], axis=-1)
    A[:, 1::2] = np.stack([u1, v1, o, z, z, z, -u2 * u1, -u2 * v1, -u2], axis=-1)
    Hn = np.linalg.svd(A)[2][:, 8].reshape(B, 3, 3)
    H21 = np.linalg.inv(T2) @ Hn @ T1
    Af = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, o], axis=-1)
    Fpre = np.linalg.svd(Af)[2][:, 8].reshape(B, 3, 3)
    U, w, Vt = np.linalg.svd(Fpre)
    w[:, 2] = 0
    F21 = T2.T @ ((U * w[:, None, :]) @ Vt) @ T1
    inv_sigma2 = 1.0 / (F64(sigma) * F64(sigma))
    h1 = np.concatenate([x1, np.ones((len(x1), 1))], axis=1)      # [N][3]
    h2 = np.concatenate([x2, np.ones((len(x2), 1))], axis=1)
    chi = np.zeros((2, B, len(pairs), 2))
    with np.errstate(all="ignore"):
        H12 = np.linalg.inv(H21)
        a = np.einsum("brc,nc->bnr", H12, h2)
        chi[0, :, :, 0] = ((x1[None] - a[..., :2] / a[..., 2:]) ** 2).sum(-1) * inv_sigma2
        a = np.einsum("brc,nc->bnr", H21, h1)
        chi[0, :, :, 1] = ((x2[None] - a[..., :2] / a[..., 2:]) ** 2).sum(-1) * inv_sigma2
        l2 = np.einsum("brc,nc->bnr", F21, h1)
        chi[1, :, :, 0] = (l2 * h2[None]).sum(-1) ** 2 / (l2[..., 0] ** 2 + l2[..., 1] ** 2) * inv_sigma2
        l1 = np.einsum("bcr,nc->bnr", F21, h2)
        chi[1, :, :, 1] = (l1 * h1[None]).sum(-1) ** 2 / (l1[..., 0] ** 2 + l1[..., 1] ** 2) * inv_sigma2
    th = np.array([F64(TH_H), F64(TH_F)])
    th_score = np.array([F64(TH_H), F64(TH_SCORE_F)])
    scores = np.zeros((2, B))
    for model in range(2):
        c = chi[model]
        scores[model] = np.where(c > th[model], 0.0, th_score[model] - c).sum(axis=(1, 2))
    best = [first_strict_maximum(scores[m]) for m in range(2)]
    return dict(scores=scores, best=[b[0] for b in best], score=[float(b[1]) for b in best], chi=chi, th=th)
