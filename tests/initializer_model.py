"""Literal model of Initializer::FindHomography and Initializer::FindFundamental (reference src/Initializer.cc:123-467, with Normalize,
:748-794) on the flat arrays of orbfe_enqueue_find_homography_fundamental (include/orbfe.h).  Every float step is an explicit np.float32 /
np.float64 operation in the reference's order; numpy arrays run ACROSS the independent hypotheses only (axis 0), never along a sum: the
double dot products, the square sums and the score are Python loops in index / match order.  It is the reference of
tests/test_initializer_model.py (against orbslam2_amd/host/Initializer.h) and tests/test_initializer_device.py (against the kernels); both
must equal it bit for bit.  find_f64() is the same pipeline in double with numpy.linalg.svd and numpy.linalg.inv.

Float contract (Q4: no contraction, IEEE divide and sqrt; the OpenCV steps are OPENCV-4.5.5-SEMANTICS, unpinned, stated in DESIGN.md
section 4l):
  normalised point          ((x - meanX) * sX, (y - meanY) * sY) in float
  rows of A                 the float products of :238-256 / :280-288; F's 8 x 9 matrix gets a zero ninth row
  cv::SVDecomp -> vt.row(8) jacobi(): the one-sided Jacobi of section 4k on 9 columns (m = 16 / 9 rows); OpenCV's own m < n path is not restated
  rank-2 step               the same Jacobi on the 3 x 3 Fpre, u = rotated rows * (float)(1 / W), w[2] = 0, (u * diag(w)) * vt
  Mat * Mat (3 x 3)         per element a double sum over k in index order, rounded once
  Mat::inv (3 x 3)          determinant and cofactors in double, det == 0 -> the zero matrix
  CheckHomography / CheckFundamental   float, left to right; 1.0 / x in double, rounded; NaN > th is false, so NaN joins the score
  score                     sequential float sum in match order; the winner is the first strict maximum above 0
"""
import numpy as np

F32, F64 = np.float32, np.float64
ERR_INVALID = -1
EPS = F64(np.finfo(F32).eps) * F64(2)   # 2 * FLT_EPSILON, as a double
FLT_MIN = F64(np.finfo(F32).tiny)
MAX_SWEEPS = 30
AS, VS = 16, 9
TH_H = F32(5.991)
TH_F, TH_SCORE_F = F32(3.841), F32(5.991)
NAN_BITS = 0x7FC00000
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


# ------------------------------------------------------------------ the Jacobi
def jacobi(At, n, m):
    """cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) for B independent m x n float matrices held transposed: At float32[B][n][16]
    (At[b][i][k] = A[k][i]).  Returns (At, Vt float32[B][n][9], W float64[B][n], info): W descending, the rows of At (rotated, not
    normalised) and Vt carried by the strict selection sort.  info = dict(sweeps[B], rotations[B], first_beta_negative[B] (-1 none), swaps[B])."""
    At = np.array(At, F32)
    B = At.shape[0]
    Vt = np.zeros((B, n, VS), F32)
    W = np.zeros((B, n), F64)
    for i in range(n):
        sd = np.zeros(B, F64)
        for k in range(m):
            sd = sd + At[:, i, k].astype(F64) * At[:, i, k].astype(F64)
        W[:, i] = sd
        Vt[:, i, i] = 1
    info = dict(sweeps=np.zeros(B, int), rotations=np.zeros(B, int), first_beta_negative=np.full(B, -1), swaps=np.zeros(B, int))
    for _ in range(MAX_SWEEPS):
        changed = np.zeros(B, bool)
        for i in range(n - 1):
            for j in range(i + 1, n):
                a, b, p = W[:, i].copy(), W[:, j].copy(), np.zeros(B, F64)
                for k in range(m):
                    p = p + At[:, i, k].astype(F64) * At[:, j, k].astype(F64)
                rot = ~(np.abs(p) <= EPS * np.sqrt(a * b))
                if not rot.any():
                    continue
                p = p * F64(2)
                beta = a - b
                gamma = np.sqrt(p * p + beta * beta)
                neg = beta < 0
                first = rot & (info["first_beta_negative"] < 0)
                info["first_beta_negative"][first] = neg[first]
                s1 = np.sqrt(((gamma - beta) * F64(0.5)) / gamma).astype(F32)
                c1 = (p / (gamma * s1.astype(F64) * F64(2))).astype(F32)
                c2 = np.sqrt((gamma + beta) / (gamma * F64(2))).astype(F32)
                s2 = (p / (gamma * c2.astype(F64) * F64(2))).astype(F32)
                c, s = np.where(neg, c1, c2)[:, None], np.where(neg, s1, s2)[:, None]
                for X, width in ((At, m), (Vt, n)):
                    xi, xj = X[:, i, :width].copy(), X[:, j, :width].copy()
                    t0 = (c * xi) + (s * xj)
                    t1 = ((-s) * xi) + (c * xj)
                    assert t0.dtype == F32
                    X[:, i, :width] = np.where(rot[:, None], t0, xi)
                    X[:, j, :width] = np.where(rot[:, None], t1, xj)
                na, nb = np.zeros(B, F64), np.zeros(B, F64)
                for k in range(m):
                    na = na + At[:, i, k].astype(F64) * At[:, i, k].astype(F64)
                    nb = nb + At[:, j, k].astype(F64) * At[:, j, k].astype(F64)
                W[:, i] = np.where(rot, na, a)
                W[:, j] = np.where(rot, nb, b)
                changed |= rot
                info["rotations"] += rot
        if not changed.any():
            break
        info["sweeps"] += changed
    for i in range(n):
        sd = np.zeros(B, F64)
        for k in range(m):
            sd = sd + At[:, i, k].astype(F64) * At[:, i, k].astype(F64)
        W[:, i] = np.sqrt(sd)
    rows = np.arange(B)
    for i in range(n - 1):
        j = np.full(B, i)
        for k in range(i + 1, n):
            j = np.where(W[rows, j] < W[:, k], k, j)
        for X in (W, At, Vt):
            tmp = X[rows, i].copy()
            X[rows, i] = X[rows, j]
            X[rows, j] = tmp
        info["swaps"] += j != i
    return At, Vt, W, info


def null_vector9(A):
    """vt.row(8) of one m x 9 float matrix (m <= 16; an 8-row matrix gets its zero ninth row here).  Returns (float32[9], info of scalars)."""
    A = np.asarray(A, F32)
    m = max(A.shape[0], 9)
    At = np.zeros((1, 9, AS), F32)
    At[0, :, :A.shape[0]] = A.T
    with np.errstate(all="ignore"):
        _, Vt, _, info = jacobi(At, 9, m)
    return Vt[0, 8, :9].copy(), {k: int(v[0]) for k, v in info.items()}


# ------------------------------------------------------------------ 3 x 3 cv::Mat steps
def mul3(a, b):
    """A cv::Mat product of [..., 3, 3] float32 arrays: per element a double sum over k in index order, rounded once."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    shape = np.broadcast_shapes(a.shape, b.shape)
    out = np.zeros(shape, F32)
    for r in range(3):
        for c in range(3):
            s = np.zeros(shape[:-2], F64)
            for k in range(3):
                s = s + a[..., r, k].astype(F64) * b[..., k, c].astype(F64)
            out[..., r, c] = s.astype(F32)
    return out


def inv3(m):
    """cv::Mat::inv() of [..., 3, 3] float32: OpenCV's closed form in double; det == 0 gives the zero matrix."""
    m = np.asarray(m, F32).astype(F64)
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = [m[..., r, c] for r in range(3) for c in range(3)]
    d = m00 * (m11 * m22 - m12 * m21) - m01 * (m10 * m22 - m12 * m20) + m02 * (m10 * m21 - m11 * m20)
    zero = d == 0
    with np.errstate(all="ignore"):
        d = F64(1.0) / d
        t = [(m11 * m22 - m12 * m21) * d, (m02 * m21 - m01 * m22) * d, (m01 * m12 - m02 * m11) * d,
             (m12 * m20 - m10 * m22) * d, (m00 * m22 - m02 * m20) * d, (m02 * m10 - m00 * m12) * d,
             (m10 * m21 - m11 * m20) * d, (m01 * m20 - m00 * m21) * d, (m00 * m11 - m01 * m10) * d]
    out = np.stack([np.where(zero, F64(0), x) for x in t], axis=-1).astype(F32)
    return out.reshape(m.shape)


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
    Fpre = Vt[:, 8, :9].reshape(B, 3, 3)
    At3 = np.zeros((B, 3, AS), F32)
    for i in range(3):
        for k in range(3):
            At3[:, i, k] = Fpre[:, k, i]
    At3, Vt3, W3, info3 = jacobi(At3, 3, 3)
    u, d = np.zeros((B, 3, 3), F32), np.zeros((B, 3, 3), F32)
    for i in range(3):
        s = np.where(W3[:, i] > FLT_MIN, (F64(1) / W3[:, i]).astype(F32), F32(0)).astype(F32)
        for k in range(3):
            u[:, k, i] = At3[:, i, k] * s
    d[:, 0, 0], d[:, 1, 1] = W3[:, 0].astype(F32), W3[:, 1].astype(F32)      # w.at<float>(2) = 0
    return mul3(mul3(u, d), Vt3[:, :, :3]), info, info3


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


def stored(score):
    """What d_all_scores holds: NaN with one bit pattern."""
    out = np.array(score, F32)
    out.view(np.uint32)[np.isnan(out)] = NAN_BITS
    return out


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
        H21 = mul3(mul3(T2inv, Hn), T1)
        H12 = inv3(H21)
        Fn, info_f, info_f3 = compute_f21(p1, p2)
        F21 = mul3(mul3(T2t, Fn), T1)
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
