"""The cv::Mat float rules that the literal models share, stated once: every float step is an explicit np.float32 /
np.float64 operation; numpy arrays run ACROSS independent problems only (the leading axes), never along a sum: dot products, square sums
and the Jacobi's loops are Python loops in index order.  tests/initializer_model.py, reconstruct_model.py, triangulate_model.py and
map_point_model.py import from here; tests/test_cvmat_model.py holds the known answers and compares orbslam2_amd/host/CvMat.h with this
module bit for bit.

  Mat * Mat                 mat(): per element a double sum over k in index order, times (double)alpha when the MatExpr carries a scale
                            (the gemm's alpha), plus a `+ C` term in double, then ONE rounding to float
  Mat::dot, cv::norm        double sums in index order; the norm takes one double sqrt
  Mat / s                   a scale by (float)(1.0 / s): a product, not a division (unit())
  Mat::inv, determinant     3 x 3: OpenCV's closed form in double; det == 0 gives the zero matrix
  cv::SVD::compute          jacobi(): one-sided (Hestenes) Jacobi on the columns, at most MAX_SWEEPS sweeps, a pair skipped when
                            |p| <= EPS * sqrt(a * b), c and s from either branch of beta, the strict selection sort; u from the rotated
                            rows times (float)(1 / W), 0 when W <= FLT_MIN (svd3())
  stored floats             a NaN is stored as NAN_BITS (stored())
"""
import numpy as np

F32, F64 = np.float32, np.float64
EPS = F64(np.finfo(F32).eps) * F64(2)   # 2 * FLT_EPSILON, as a double
FLT_MIN = F64(np.finfo(F32).tiny)
MAX_SWEEPS = 30
AS, VS = 16, 9                          # row strides of At and Vt
NAN_BITS = 0x7FC00000


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


def transposed(A, n):
    """At float32[1][n][16] of one matrix with n columns (and at most 16 rows)."""
    A = np.asarray(A, F32)
    At = np.zeros((1, n, AS), F32)
    At[0, :, :A.shape[0]] = A.T
    return At


def null_vector(A):
    """vt.row(n - 1) of one m x n float matrix (m <= 16; fewer than n rows are padded with zero rows to n).  Returns (float32[n], info of
    scalars; first_beta_negative is None when nothing rotated)."""
    A = np.asarray(A, F32)
    n = A.shape[1]
    with np.errstate(all="ignore"):
        _, Vt, _, info = jacobi(transposed(A, n), n, max(A.shape[0], n))
    info = {k: int(v[0]) for k, v in info.items()}
    info["first_beta_negative"] = None if info["first_beta_negative"] < 0 else bool(info["first_beta_negative"])
    return Vt[0, n - 1, :n].copy(), info


# ------------------------------------------------------------------ cv::Mat steps
def mat(a, b, alpha=None, plus=None):
    """A cv::Mat product a[..., R, K] * b[..., K, C] (float32; the leading axes are independent problems and broadcast): per element a
    double sum over k in index order, times (double)alpha when given, plus (double)plus[..., R, C] when given, rounded once."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    lead = np.broadcast_shapes(a.shape[:-2], b.shape[:-2])
    out = np.zeros(lead + (a.shape[-2], b.shape[-1]), F32)
    for r in range(a.shape[-2]):
        for c in range(b.shape[-1]):
            s = np.zeros(lead, F64)
            for k in range(a.shape[-1]):
                s = s + a[..., r, k].astype(F64) * b[..., k, c].astype(F64)
            if alpha is not None:
                s = F64(alpha) * s
            if plus is not None:
                s = s + np.asarray(plus, F32)[..., r, c].astype(F64)
            out[..., r, c] = s.astype(F32)
    return out


def det3(m):
    """cv::determinant of [..., 3, 3] float32: the double expression d of the closed inverse."""
    m = np.asarray(m, F32).astype(F64)
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = [m[..., r, c] for r in range(3) for c in range(3)]
    return m00 * (m11 * m22 - m12 * m21) - m01 * (m10 * m22 - m12 * m20) + m02 * (m10 * m21 - m11 * m20)


def inv3(m):
    """cv::Mat::inv() of [..., 3, 3] float32: OpenCV's closed form in double; det == 0 gives the zero matrix."""
    d = det3(m)
    m = np.asarray(m, F32).astype(F64)
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = [m[..., r, c] for r in range(3) for c in range(3)]
    zero = d == 0
    with np.errstate(all="ignore"):
        d = F64(1.0) / d
        t = [(m11 * m22 - m12 * m21) * d, (m02 * m21 - m01 * m22) * d, (m01 * m12 - m02 * m11) * d,
             (m12 * m20 - m10 * m22) * d, (m00 * m22 - m02 * m20) * d, (m02 * m10 - m00 * m12) * d,
             (m10 * m21 - m11 * m20) * d, (m01 * m20 - m00 * m21) * d, (m00 * m11 - m01 * m10) * d]
    out = np.stack([np.where(zero, F64(0), x) for x in t], axis=-1).astype(F32)
    return out.reshape(m.shape)


def svd3(A):
    """cv::SVD::compute of [B][3][3] float32: (u float32[B][3][3], w float32[B][3], vt float32[B][3][3], info of the Jacobi);
    w[i] = (float)W[i], u[k][i] = At[i][k] * (float)(1 / W[i]), 0 when W[i] <= FLT_MIN (the basis completion is not restated)."""
    A = np.asarray(A, F32)
    B = A.shape[0]
    At = np.zeros((B, 3, AS), F32)
    for i in range(3):
        for k in range(3):
            At[:, i, k] = A[:, k, i]
    At, Vt, W, info = jacobi(At, 3, 3)
    u = np.zeros((B, 3, 3), F32)
    for i in range(3):
        s = np.where(W[:, i] > FLT_MIN, (F64(1) / W[:, i]).astype(F32), F32(0)).astype(F32)
        for k in range(3):
            u[:, k, i] = At[:, i, k] * s
    return u, W.astype(F32), Vt[:, :, :3].copy(), info


def norm(v):
    """cv::norm of float32[..., n] vectors: a double sum of double squares in index order, one sqrt."""
    v = np.asarray(v, F32)
    s = np.zeros(v.shape[:-1], F64)
    for k in range(v.shape[-1]):
        s = s + v[..., k].astype(F64) * v[..., k].astype(F64)
    return np.sqrt(s)


def unit(t):
    """t / cv::norm(t) of one vector: a scale by (float)(1.0 / norm); no zero test."""
    return (np.asarray(t, F32) * F32(F64(1.0) / norm(t))).astype(F32)


def stored(a):
    """What an output array holds: NaN with one bit pattern."""
    out = np.array(a, F32)
    out.view(np.uint32)[np.isnan(out)] = NAN_BITS
    return out
