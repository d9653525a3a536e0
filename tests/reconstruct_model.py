"""Literal model of Initializer::ReconstructF / ReconstructH / DecomposeE / CheckRT / Triangulate (reference src/Initializer.cc:469-746,
:797-928) on the flat arrays of orbfe_enqueue_reconstruct_initial (include/orbfe.h).  Every float step is an explicit np.float32 /
np.float64 operation in the reference's order; numpy arrays run ACROSS the independent matches only (axis 0), never along a sum.  The
cv::Mat steps and the Jacobi (with 4 and 3 columns) are tests/cvmat_model.py's.  It is the reference of
tests/test_reconstruct_model.py (against orbslam2_amd/host/Initializer.h) and tests/test_reconstruct_device.py (against the kernels);
both must equal it bit for bit.  reconstruct_f64() is the same pipeline in double with numpy.linalg.svd / inv / det.

Float contract (Q4; the OpenCV steps are OPENCV-4.5.5-SEMANTICS, unpinned, stated in DESIGN.md section 4m):
  model                     RH = SH / (SH + SF) in float, H when (double)RH > 0.40
  Mat * Mat                 per element a double sum over k in index order (+ a `+ t` term in double), rounded once; a MatExpr scale
                            (s * U * Rp, -R.t() * t) is the gemm's alpha: the double sum times (double)alpha, then the one rounding
  K.inv(), determinant      inv3(), det3(): the closed 3 x 3 form in double
  3 x 3 SVD                 svd3(): the Jacobi; w[i] = (float)W[i]; u[k][i] = At[i][k] * (float)(1 / W[i]), 0 when W[i] <= FLT_MIN
  t / norm(t), x3D / w      scales by (float)(1.0 / d); no zero test
  rows of Triangulate's A   x * P.row(2) - P.row(0) in float, the product rounded, then the difference
  CheckRT                   literal (see check_rt)
  sorted cosine             the order of the keys `order_key`: that of the floats, -0 before +0, any NaN after every number
  stored floats             a NaN is stored as 0x7fc00000
"""
import numpy as np

from tests import initializer_model as M
from tests.cvmat_model import AS, F32, F64, NAN_BITS, det3, inv3, jacobi, mat, norm, stored, svd3, unit  # noqa: F401 (NAN_BITS is read through this module)

ERR_INVALID = -1
COS_NONE = F32(2.0)
H_MODEL, F_MODEL = 0, 1
MAX_MATCHES, MAX_KEYS = M.MAX_MATCHES, M.MAX_KEYS


def k_matrix(K4):
    K = np.zeros((3, 3), F32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2], K[2, 2] = K4[0], K4[1], K4[2], K4[3], 1
    return K


def _svd3(A):
    """cv::SVD::compute of one 3 x 3 float matrix: (u, w float32[3], vt)."""
    u, w, vt, _ = svd3(A[None])
    return u[0], w[0], vt[0]


def decompose_e(F21, K4):
    """ReconstructF's four motion hypotheses (:478-496) in the reference's order."""
    K = k_matrix(K4)
    E = mat(mat(K.T, F21), K)
    u, _, vt = _svd3(E)
    t = unit(u[:, 2])
    Wm = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], F32)
    R1 = mat(mat(u, Wm), vt)
    if det3(R1) < 0:
        R1 = -R1
    R2 = mat(mat(u, Wm.T), vt)
    if det3(R2) < 0:
        R2 = -R2
    return [R1, R2, R1, R2], [t, t, -t, -t]


def decompose_h(H21, K4):
    """ReconstructH's eight motion hypotheses (:583-685): (early, vR, vt); early = 2 under the test of :596."""
    K = k_matrix(K4)
    A = mat(mat(inv3(K), H21), K)
    U, w, Vt = _svd3(A)
    s = F32(det3(U) * det3(Vt))
    d1, d2, d3 = w[0], w[1], w[2]
    if F64(d1 / d2) < 1.00001 or F64(d2 / d3) < 1.00001:
        return 2, [], []
    aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
    aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
    x1, x3 = [aux1, aux1, -aux1, -aux1], [aux3, -aux3, aux3, -aux3]
    aux_stheta = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2)
    ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
    stheta = [aux_stheta, -aux_stheta, -aux_stheta, aux_stheta]
    aux_sphi = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2)
    cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
    sphi = [aux_sphi, -aux_sphi, -aux_sphi, aux_sphi]
    assert all(type(x) is F32 for x in (aux1, aux3, aux_stheta, ctheta, aux_sphi, cphi, s))
    vR, vt = [], []
    for i in range(8):
        Rp = np.eye(3, dtype=F32)
        if i < 4:
            Rp[0, 0], Rp[0, 2], Rp[2, 0], Rp[2, 2] = ctheta, -stheta[i], stheta[i], ctheta
            tp = np.array([x1[i], 0, -x3[i]], F32) * F32(d1 - d3)
        else:
            Rp[0, 0], Rp[0, 2], Rp[1, 1], Rp[2, 0], Rp[2, 2] = cphi, sphi[i - 4], -1, sphi[i - 4], -cphi
            tp = np.array([x1[i - 4], 0, x3[i - 4]], F32) * F32(d1 + d3)
        vR.append(mat(mat(U, Rp, alpha=s), Vt))
        vt.append(unit(mat(U, tp[:, None])[:, 0]))
    return 0, vR, vt


def camera2(R, t, K4):
    """P2 = K [R|t] (3 x 4) and O2 = -R.t() * t of CheckRT (:819-825)."""
    Rt = np.concatenate([R, np.asarray(t, F32)[:, None]], axis=1)
    return mat(k_matrix(K4), Rt), mat(R.T, np.asarray(t, F32)[:, None], alpha=-1.0)[:, 0]


def check_rt(R, t, K4, x1, y1, x2, y2, inlier, th2):
    """CheckRT (:797-906) of one hypothesis over n matches (float32[n] coordinates, bool[n] inlier).  Returns (codes uint8[n],
    cos float32[n], p float32[n][3], q: the tested quantities for the margins of the float64 comparison)."""
    fx, fy, cx, cy = [F32(x) for x in K4]
    K = k_matrix(K4)
    P1 = np.zeros((3, 4), F32)
    P1[:, :3] = K
    P2, O2 = camera2(R, t, K4)
    n = len(x1)
    At = np.zeros((n, 4, AS), F32)
    for c in range(4):
        At[:, c, 0] = x1 * P1[2, c] - P1[0, c]
        At[:, c, 1] = y1 * P1[2, c] - P1[1, c]
        At[:, c, 2] = x2 * P2[2, c] - P2[0, c]
        At[:, c, 3] = y2 * P2[2, c] - P2[1, c]
    assert At.dtype == F32
    _, Vt, _, _ = jacobi(At, 4, 4)
    v = Vt[:, 3, :4]
    p = v[:, :3] * (F64(1.0) / v[:, 3].astype(F64)).astype(F32)[:, None]
    finite = np.isfinite(p).all(axis=1)
    dist1 = norm(p).astype(F32)                     # normal1 = p3dC1 - O1, O1 = 0
    n2 = p - O2[None, :]
    dist2 = norm(n2).astype(F32)
    dot = np.zeros(n, F64)
    for k in range(3):
        dot = dot + p[:, k].astype(F64) * n2[:, k].astype(F64)
    cos = (dot / (dist1 * dist2).astype(F64)).astype(F32)
    low = cos.astype(F64) < 0.99998
    p2 = mat(R, p[:, :, None], plus=np.asarray(t, F32)[:, None])[:, :, 0]      # R * p3dC1 + t
    inv1 = (F64(1.0) / p[:, 2].astype(F64)).astype(F32)
    ex, ey = ((fx * p[:, 0]) * inv1 + cx) - x1, ((fy * p[:, 1]) * inv1 + cy) - y1
    err1 = ex * ex + ey * ey
    inv2 = (F64(1.0) / p2[:, 2].astype(F64)).astype(F32)
    ex, ey = ((fx * p2[:, 0]) * inv2 + cx) - x2, ((fy * p2[:, 1]) * inv2 + cy) - y2
    err2 = ex * ex + ey * ey
    assert err1.dtype == F32 and err2.dtype == F32 and p.dtype == F32 and n2.dtype == F32
    codes = np.select([~inlier, ~finite, (p[:, 2] <= 0) & low, (p2[:, 2] <= 0) & low, err1 > th2, err2 > th2, ~low],
                      [0, 1, 2, 3, 4, 5, 6], 7).astype(np.uint8)
    return codes, cos, p, dict(z1=p[:, 2], z2=p2[:, 2], err1=err1, err2=err2, cos=cos, w=v[:, 3].copy())


def order_key(cos):
    """uint32 keys whose order is the sorted order of the cosines: the floats' own, -0 before +0, any NaN last."""
    b = np.ascontiguousarray(cos, F32).view(np.uint32)
    k = np.where(b >> 31, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(cos), np.uint32(0xFFFFFFFF), k).astype(np.uint32)


def kth_cosine(cos, counted):
    """vCosParallax[min(50, size - 1)] after the sort (:897-900), or 2.0 when nothing was counted."""
    c = cos[counted]
    if len(c) == 0:
        return COS_NONE
    c = c[np.argsort(order_key(c), kind="stable")]
    return stored(c[min(50, len(c) - 1)])[()]


def choose_f(ngood, n_inliers, min_triangulated):
    """The count rules of ReconstructF (:498-566): the chosen hypothesis or -1."""
    max_good = max(ngood[:4])
    n_min_good = max(int(0.9 * n_inliers), min_triangulated)
    nsimilar = sum(1 for g in ngood[:4] if g > 0.7 * max_good)
    if max_good < n_min_good or nsimilar > 1:
        return -1
    return [int(g) for g in ngood[:4]].index(max_good)


def choose_h(ngood, n_inliers, min_triangulated):
    """ReconstructH (:688-720) without the parallax term."""
    best, second, idx = 0, 0, -1
    for i in range(8):
        if ngood[i] > best:
            second, best, idx = best, int(ngood[i]), i
        elif ngood[i] > second:
            second = int(ngood[i])
    return idx if second < 0.75 * best and best > min_triangulated and best > 0.9 * n_inliers else -1


def refused(n1, n2, N, K4, sigma, min_triangulated, model):
    return (N < 1 or N > MAX_MATCHES or n1 < 0 or n2 < 0 or n1 > MAX_KEYS or n2 > MAX_KEYS or not sigma > 0 or not K4[0] > 0 or not K4[1] > 0
            or min_triangulated < 0 or model not in (-1, 0, 1))


def accept(model, cos_parallax, min_parallax):
    """ReconstructAccept of Initializer.h: the parallax test that stays on the host."""
    parallax = F32(0) if cos_parallax == COS_NONE else F32(F64(F32(np.arccos(F32(cos_parallax))) * F32(180)) / F64(np.pi))
    return bool(parallax >= min_parallax) if model == H_MODEL else bool(parallax > min_parallax)


def reconstruct(keys1, keys2, pairs, H21, F21, score, best, inliers_h, inliers_f, K4, sigma, min_triangulated=50, model=-1):
    """orbfe_enqueue_reconstruct_initial on numpy arrays.  Returns dict(status, model, hyp_R float32[8][9] / hyp_t float32[8][3] with
    nhyp rows valid, nhyp, ngood int32[8], cos_parallax float32[8], result, choice, R21 / t21 (None: untouched), p3d float32[n1][3],
    triangulated uint8[n1], codes uint8[8][N], n_inliers, q (per hypothesis, the tested quantities))."""
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    n1, n2, N = len(keys1), len(keys2), len(pairs)
    K4 = np.asarray(K4, F32)
    assert not refused(n1, n2, N, K4, sigma, min_triangulated, model)
    sigma = F32(sigma)
    out = dict(status=0, hyp_R=np.zeros((8, 9), F32), hyp_t=np.zeros((8, 3), F32), nhyp=0, ngood=np.zeros(8, np.int32), cos_parallax=np.full(8, COS_NONE, F32),
               result=0, choice=-1, R21=None, t21=None, p3d=np.zeros((n1, 3), F32), triangulated=np.zeros(n1, np.uint8), codes=np.zeros((8, N), np.uint8), q=[])
    with np.errstate(all="ignore"):
        if model == -1:
            SH, SF = F32(score[0]), F32(score[1])
            RH = SH / (SH + SF)
            assert type(RH) is F32
            model = H_MODEL if F64(RH) > 0.40 else F_MODEL
        out["model"] = model
        pair_ok = (pairs[:, 0] >= 0) & (pairs[:, 0] < n1) & (pairs[:, 1] >= 0) & (pairs[:, 1] < n2)
        if not pair_ok.all():
            out["status"] = ERR_INVALID
        flags = np.asarray(inliers_h if model == H_MODEL else inliers_f, np.uint8) != 0
        out["n_inliers"] = n_inl = int(flags.sum())
        if best[model] < 0:
            out["result"] = 1
            return out
        if model == H_MODEL:
            early, vR, vt = decompose_h(np.asarray(H21, F32).reshape(3, 3), K4)
            if early:
                out["result"] = early
                return out
        else:
            vR, vt = decompose_e(np.asarray(F21, F32).reshape(3, 3), K4)
        out["nhyp"] = nhyp = len(vR)
        i1, i2 = np.where(pair_ok, pairs[:, 0], 0), np.where(pair_ok, pairs[:, 1], 0)
        if n1 == 0 or n2 == 0:
            x1 = y1 = x2 = y2 = np.zeros(N, F32)
        else:
            x1, y1, x2, y2 = keys1["x"][i1].astype(F32), keys1["y"][i1].astype(F32), keys2["x"][i2].astype(F32), keys2["y"][i2].astype(F32)
        th2 = F32(F64(4.0) * F64(sigma * sigma))
        pts = []
        for h in range(nhyp):
            out["hyp_R"][h], out["hyp_t"][h] = stored(vR[h].reshape(9)), stored(vt[h])
            codes, cos, p, q = check_rt(vR[h], vt[h], K4, x1, y1, x2, y2, flags & pair_ok, th2)
            out["codes"][h] = codes
            out["ngood"][h] = int((codes >= 6).sum())
            out["cos_parallax"][h] = kth_cosine(cos, codes >= 6)
            out["q"].append(q)
            pts.append(p)
        choice = (choose_h if model == H_MODEL else choose_f)(out["ngood"], n_inl, min_triangulated)
        out["choice"] = choice
        if choice < 0:
            out["result"] = 3
            return out
        out["R21"], out["t21"] = out["hyp_R"][choice].copy(), out["hyp_t"][choice].copy()
        for i in range(N):          # match order; mvMatches12 names every first keypoint once
            if out["codes"][choice, i] >= 6:
                out["p3d"][pairs[i, 0]] = pts[choice][i]
                out["triangulated"][pairs[i, 0]] = out["codes"][choice, i] == 7
        return out


# ------------------------------------------------------------------ the float64 restatement
def reconstruct_f64(keys1, keys2, pairs, H21, F21, flags, K4, sigma, model, min_triangulated=50):
    """The same stage in double with numpy.linalg (no faulty indices, a model given).  Returns dict(result, R[nhyp][3][3], t[nhyp][3],
    codes[nhyp][N], q (per hypothesis: z1, z2, err1, err2, cos and the distances r1, r2), p[nhyp][N][3], ngood, choice, th2)."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    fx, fy, cx, cy = [float(x) for x in K4]
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
    flags = np.asarray(flags) != 0
    x1 = np.stack([keys1["x"][pairs[:, 0]], keys1["y"][pairs[:, 0]]], axis=1).astype(F64)
    x2 = np.stack([keys2["x"][pairs[:, 1]], keys2["y"][pairs[:, 1]]], axis=1).astype(F64)
    out = dict(result=0, choice=-1, th2=4.0 * float(sigma) ** 2)
    if model == F_MODEL:
        E = K.T @ np.asarray(F21, F64).reshape(3, 3) @ K
        u, _, vt = np.linalg.svd(E)
        t = u[:, 2] / np.linalg.norm(u[:, 2])
        Wm = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])
        R1, R2 = u @ Wm @ vt, u @ Wm.T @ vt
        R1, R2 = (R1 if np.linalg.det(R1) > 0 else -R1), (R2 if np.linalg.det(R2) > 0 else -R2)
        vR, vT = [R1, R2, R1, R2], [t, t, -t, -t]
    else:
        A = np.linalg.inv(K) @ np.asarray(H21, F64).reshape(3, 3) @ K
        U, w, Vt = np.linalg.svd(A)
        s = np.linalg.det(U) * np.linalg.det(Vt)
        d1, d2, d3 = w
        if d1 / d2 < 1.00001 or d2 / d3 < 1.00001:
            out["result"] = 2
            return out
        aux1, aux3 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3)), np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
        x1s, x3s = [aux1, aux1, -aux1, -aux1], [aux3, -aux3, aux3, -aux3]
        root = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3))
        ast, ct = root / ((d1 + d3) * d2), (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
        asp, cp = root / ((d1 - d3) * d2), (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
        sg = [1, -1, -1, 1]
        vR, vT = [], []
        for i in range(8):
            j = i % 4
            if i < 4:
                Rp = np.array([[ct, 0, -sg[j] * ast], [0, 1, 0], [sg[j] * ast, 0, ct]])
                tp = np.array([x1s[j], 0, -x3s[j]]) * (d1 - d3)
            else:
                Rp = np.array([[cp, 0, sg[j] * asp], [0, -1, 0], [sg[j] * asp, 0, -cp]])
                tp = np.array([x1s[j], 0, x3s[j]]) * (d1 + d3)
            tt = U @ tp
            vR.append(s * U @ Rp @ Vt)
            vT.append(tt / np.linalg.norm(tt))
    nh, N = len(vR), len(pairs)
    out.update(R=np.array(vR), t=np.array(vT), codes=np.zeros((nh, N), np.uint8), p=np.zeros((nh, N, 3)), q=[])
    P1 = np.concatenate([K, np.zeros((3, 1))], axis=1)
    with np.errstate(all="ignore"):
        for h in range(nh):
            R, t = vR[h], vT[h]
            P2 = K @ np.concatenate([R, t[:, None]], axis=1)
            O2 = -R.T @ t
            A = np.stack([x1[:, :1] * P1[2] - P1[0], x1[:, 1:] * P1[2] - P1[1], x2[:, :1] * P2[2] - P2[0], x2[:, 1:] * P2[2] - P2[1]], axis=1)
            v = np.linalg.svd(A)[2][:, 3]
            p = v[:, :3] / v[:, 3:]
            n2 = p - O2
            cos = (p * n2).sum(1) / (np.linalg.norm(p, axis=1) * np.linalg.norm(n2, axis=1))
            low = cos < 0.99998
            p2 = p @ R.T + t
            err1 = (fx * p[:, 0] / p[:, 2] + cx - x1[:, 0]) ** 2 + (fy * p[:, 1] / p[:, 2] + cy - x1[:, 1]) ** 2
            err2 = (fx * p2[:, 0] / p2[:, 2] + cx - x2[:, 0]) ** 2 + (fy * p2[:, 1] / p2[:, 2] + cy - x2[:, 1]) ** 2
            out["codes"][h] = np.select([~flags, ~np.isfinite(p).all(1), (p[:, 2] <= 0) & low, (p2[:, 2] <= 0) & low, err1 > out["th2"], err2 > out["th2"], ~low],
                                        [0, 1, 2, 3, 4, 5, 6], 7)
            out["p"][h] = p
            out["q"].append(dict(z1=p[:, 2], z2=p2[:, 2], err1=err1, err2=err2, cos=cos, r1=np.linalg.norm(p, axis=1), r2=np.linalg.norm(p2, axis=1)))
    out["ngood"] = (out["codes"] >= 6).sum(axis=1)
    ng = np.concatenate([out["ngood"], np.zeros(8 - nh, int)])
    out["choice"] = (choose_h if model == H_MODEL else choose_f)(ng, int(flags.sum()), min_triangulated)
    if out["choice"] < 0:
        out["result"] = 3
    return out
