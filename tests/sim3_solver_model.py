"""The model of Sim3Solver (reference src/Sim3Solver.cc) as orbfe_enqueue_sim3_ransac_batch (orbslam2_amd/csrc/orbfe_sim3_ransac.hip) and
orbslam2_amd/host/Sim3Solver.h compute it: numpy, every float32 step a float32 operation in the stated order, every double sum a chain of
Python floats, the Jacobi scalar float64.  Arrays run across correspondences (element by element) only, never along a sum.  DESIGN.md
section 4o states the arithmetic step by step; the rules of section 4i2 that tests/cvmat_model.py does not hold (cv::reduce, cv::pow, den,
ms12i) are defined here once.

reference_errors() is the float64 path shaped like the reference (np.linalg.eigh, the angle-axis of :275-285, Rodrigues), the yardstick
of tests/test_sim3_solver_model.py; Solver is a literal transcription of Sim3Solver::iterate (:141-208) fed per-hypothesis results."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
ERR_INVALID = -1
RAND_MAX = 2147483647
JACOBI_SWEEPS = 30
THIRD = f32(1.0 / 3)                    # `/ P.cols`: a scale by (float)(1.0 / 3)
NAN_BITS = 0x7fc00000                   # the one stored NaN
HYP_DTYPE = np.dtype([("n_inliers", "<i4"), ("s12", "<f4"), ("R12", "<f4", (9,)), ("t12", "<f4", (3,)), ("pad", "<i4", (2,))])
assert HYP_DTYPE.itemsize == 64


def stored(a):
    """float32 array with every NaN as the one bit pattern."""
    a = np.array(a, f32)
    u = a.view(np.uint32)
    u[np.isnan(a)] = NAN_BITS
    return a


# ------------------------------------------------------------------------------------------------ draws and the iteration count
def random_int(r, d):
    """DUtils::Random::RandomInt(0, d - 1) on the raw rand() value r (Thirdparty/DLib/src/Random.cpp:47-50)."""
    return int((float(r) / 2147483648.0) * d)


def draw_set(r3, N):
    """The three correspondences of :164-178 from three raw rand() values: vAvailableIndices = 0 .. N-1, each draw swaps with the back
    and pops.  Only the drawn positions ever differ from the identity, so no array is kept."""
    r0 = random_int(r3[0], N)
    i0 = r0                                                   # position r0 now holds N - 1
    r1 = random_int(r3[1], N - 1)
    i1 = N - 1 if r1 == r0 else r1
    back = N - 1 if r0 == N - 2 else N - 2                    # what position N - 2 holds: moved to position r1
    r2 = random_int(r3[2], N - 2)
    i2 = back if r2 == r1 else (N - 1 if r2 == r0 else r2)
    return i0, i1, i2


def iterations_for(N, prob, min_inliers, max_its):
    """SetRansacParameters (:115-139) for N correspondences; 0 is the bNoMore exit of :147-151."""
    if N < min_inliers:
        return 0
    if N == min_inliers:
        n = 1.0
    else:
        eps = float(f32(min_inliers) / f32(N))
        with np.errstate(all="ignore"):
            den = math.log(1 - math.pow(eps, 3))
            n = math.ceil(math.log(1 - prob) / den) if den != 0 else math.inf
    n = max_its if not n < max_its else int(n)                # the clamp before the conversion: no overflow
    return max(1, min(n, max_its))


def its_table(max_pairs, prob, min_inliers, max_its):
    return np.array([iterations_for(N, prob, min_inliers, max_its) for N in range(max_pairs + 1)], np.int32)


# ------------------------------------------------------------------------------------------------ the constructor's filter (:63-110)
def gate(sigma2):
    """mvnMaxError: a std::vector<size_t>, so 9.210 * sigma2 is truncated; compared as float."""
    return f32(int(9.210 * float(f32(sigma2))))


def _row_dot_plus(T, X):
    """Rcw * Xw + tcw: per row a double sum over k in index order plus t, rounded once.  X is [n][3] float32."""
    T = np.asarray(T, f32).reshape(3, 4).astype(f64)
    X = X.astype(f64)
    return np.stack([(((T[r, 0] * X[:, 0] + T[r, 1] * X[:, 1]) + T[r, 2] * X[:, 2]) + T[r, 3]).astype(f32) for r in range(3)], axis=1)


def _to_image(Xc, cam):
    fx, fy, cx, cy = (f32(v) for v in cam)
    with np.errstate(all="ignore"):
        invz = f32(1) / Xc[:, 2]
        x, y = Xc[:, 0] * invz, Xc[:, 1] * invz
        return np.stack([fx * x + cx, fy * y + cy], axis=1).astype(f32)


def filter_pairs(s):
    """(status, corr [N][2], table): the surviving pairs in pair order and per survivor X3Dc1, X3Dc2, P1im1, P2im2 and both gates."""
    n1, n2, nlev = len(s["keys1"]), len(s["keys2"]), len(s["sigma2"])
    status, keep = 0, []
    for i1, i2 in np.asarray(s["pairs"], np.int64).reshape(-1, 2):
        ok = 0 <= i1 < n1 and 0 <= i2 < n2
        if ok:
            ok = 0 <= s["keys1"]["octave"][i1] < nlev and 0 <= s["keys2"]["octave"][i2] < nlev
        if not ok:
            status = ERR_INVALID
            continue
        if s["valid1"][i1] and s["valid2"][i2]:
            keep.append((i1, i2))
    corr = np.array(keep, np.int32).reshape(-1, 2)
    X1 = _row_dot_plus(s["T1w"], np.asarray(s["pos1"], f32).reshape(-1, 3)[corr[:, 0]])
    X2 = _row_dot_plus(s["T2w"], np.asarray(s["pos2"], f32).reshape(-1, 3)[corr[:, 1]])
    g1 = np.array([gate(s["sigma2"][s["keys1"]["octave"][i]]) for i in corr[:, 0]], f32)
    g2 = np.array([gate(s["sigma2"][s["keys2"]["octave"][i]]) for i in corr[:, 1]], f32)
    return status, corr, dict(X1=X1, X2=X2, p1=_to_image(X1, s["cam"]), p2=_to_image(X2, s["cam"]), g1=g1, g2=g2)


# ------------------------------------------------------------------------------------------------ ComputeSim3 (:227-338)
def _matmul(a, b, alpha=None, plus=None):
    """A cv::Mat float product: per element a double sum over k in index order, times alpha, plus C, rounded once."""
    R, K, Cc = len(a), len(b), len(b[0])
    out = np.zeros((R, Cc), f32)
    for r in range(R):
        for c in range(Cc):
            sm = 0.0
            for k in range(K):
                sm += float(a[r][k]) * float(b[k][c])
            if alpha is not None:
                sm = alpha * sm
            if plus is not None:
                sm += float(plus[r][c])
            out[r, c] = f32(sm)
    return out


def centroid(P):
    """ComputeCentroid (:216-225): cv::reduce(SUM) is a float sum in index order, `/ P.cols` a scale by (float)(1.0 / 3)."""
    C = np.array([((P[r, 0] + P[r, 1]) + P[r, 2]) * THIRD for r in range(3)], f32)
    return (P - C[:, None]).astype(f32), C


def horn_n(M):
    """Step 3: the entries are float expressions, left to right."""
    n11 = (M[0, 0] + M[1, 1]) + M[2, 2]
    n12 = M[1, 2] - M[2, 1]
    n13 = M[2, 0] - M[0, 2]
    n14 = M[0, 1] - M[1, 0]
    n22 = (M[0, 0] - M[1, 1]) - M[2, 2]
    n23 = M[0, 1] + M[1, 0]
    n24 = M[2, 0] + M[0, 2]
    n33 = (-M[0, 0] + M[1, 1]) - M[2, 2]
    n34 = M[1, 2] + M[2, 1]
    n44 = (-M[0, 0] - M[1, 1]) + M[2, 2]
    return np.array([[n11, n12, n13, n14], [n12, n22, n23, n24], [n13, n23, n33, n34], [n14, n24, n34, n44]], f32)


def jacobi4(N):
    """Cyclic two-sided Jacobi on the float entries of the symmetric 4 x 4 N, in double: pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), at
    most JACOBI_SWEEPS sweeps, ended by the first sweep that rotates nothing.  A pair is skipped (and its entry set to 0) when adding
    |a_pq| changes neither |a_pp| nor |a_qq|.  sqrt and divide only.  Returns (diagonal, V with the eigenvectors as columns, sweeps)."""
    A = [[float(N[i][j]) for j in range(4)] for i in range(4)]
    V = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    sweeps = 0
    for _ in range(JACOBI_SWEEPS):
        rotated = False
        for p in range(3):
            for q in range(p + 1, 4):
                apq = A[p][q]
                g = abs(apq)
                if abs(A[p][p]) + g == abs(A[p][p]) and abs(A[q][q]) + g == abs(A[q][q]):
                    A[p][q] = A[q][p] = 0.0
                    continue
                theta = (A[q][q] - A[p][p]) / (2.0 * apq)
                t = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0))
                if theta < 0:
                    t = -t
                c = 1.0 / math.sqrt(t * t + 1.0)
                sn = t * c
                A[p][p] = A[p][p] - t * apq
                A[q][q] = A[q][q] + t * apq
                A[p][q] = A[q][p] = 0.0
                for r in range(4):
                    if r != p and r != q:
                        arp, arq = A[r][p], A[r][q]
                        A[r][p] = A[p][r] = c * arp - sn * arq
                        A[r][q] = A[q][r] = sn * arp + c * arq
                for r in range(4):
                    vrp, vrq = V[r][p], V[r][q]
                    V[r][p] = c * vrp - sn * vrq
                    V[r][q] = sn * vrp + c * vrq
                rotated = True
        if not rotated:
            break
        sweeps += 1
    return [A[i][i] for i in range(4)], V, sweeps


def quat_rotation(w, x, y, z):
    """The rotation matrix of the quaternion (w, x, y, z) / |.| in double, each entry rounded once.  A zero vector part gives I."""
    ww, xx, yy, zz = w * w, x * x, y * y, z * z
    xy, xz, yz, wx, wy, wz = x * y, x * z, y * z, w * x, w * y, w * z
    n = ((ww + xx) + yy) + zz
    R = [(((ww + xx) - yy) - zz) / n, (2.0 * (xy - wz)) / n, (2.0 * (xz + wy)) / n,
         (2.0 * (xy + wz)) / n, (((ww - xx) + yy) - zz) / n, (2.0 * (yz - wx)) / n,
         (2.0 * (xz - wy)) / n, (2.0 * (yz + wx)) / n, (((ww - xx) - yy) + zz) / n]
    return np.array(R, f64).astype(f32).reshape(3, 3)


def compute_sim3(P1, P2, fix_scale):
    """ComputeSim3 on two 3 x 3 float32 matrices whose columns are the drawn points.  Returns R, t, s, sR, sRinv, tinv (float32)."""
    with np.errstate(all="ignore"):
        Pr1, O1 = centroid(P1)
        Pr2, O2 = centroid(P2)
        M = _matmul(Pr2, Pr1.T)
        d, V, _ = jacobi4(horn_n(M))
        top = 0
        for i in range(1, 4):
            if d[i] > d[top]:                                # first strict maximum
                top = i
        R = quat_rotation(V[0][top], V[1][top], V[2][top], V[3][top])
        P3 = _matmul(R, Pr2)
        if fix_scale:
            s = f32(1.0)
        else:
            nom = 0.0
            for r in range(3):
                for c in range(3):
                    nom += float(Pr1[r, c]) * float(P3[r, c])          # Mat::dot: a double sum
            aux = (P3 * P3).astype(f32)                                 # cv::pow(., 2): a float product
            den = 0.0
            for r in range(3):
                for c in range(3):
                    den += float(aux[r, c])                             # a double sum of float squares
            s = f32(f64(nom) / f64(den))
        t = _matmul(R, O2.reshape(3, 1), alpha=-float(s), plus=O1.reshape(3, 1)).reshape(3)   # O1 - s * R * O2: one gemm
        sR = (s * R).astype(f32)
        sRinv = (R.T * f32(f64(1.0) / f64(s))).astype(f32)              # (1.0 / s) * R.t(): a scale by (float)(1.0 / s)
        tinv = _matmul(sRinv, t.reshape(3, 1), alpha=-1.0).reshape(3)
    return R, t, s, sR, sRinv, tinv


def _project(X, sR, t, cam):
    """Sim3Solver::Project (:383-404) on [n][3] float32 points."""
    A = sR.astype(f64); X = X.astype(f64)
    with np.errstate(all="ignore"):
        P = np.stack([(((A[r, 0] * X[:, 0] + A[r, 1] * X[:, 1]) + A[r, 2] * X[:, 2]) + f64(t[r])).astype(f32) for r in range(3)], axis=1)
    return _to_image(P, cam)


def _sq(d):
    d = d.astype(f64)
    with np.errstate(all="ignore"):
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(f32)


def check_inliers(tab, sR, t, sRinv, tinv, cam):
    """CheckInliers (:341-365): (inlier flags, err1, err2)."""
    with np.errstate(all="ignore"):
        e1 = _sq(tab["p1"] - _project(tab["X2"], sR, t, cam))
        e2 = _sq(_project(tab["X1"], sRinv, tinv, cam) - tab["p2"])
        return (e1 < tab["g1"]) & (e2 < tab["g2"]), e1, e2


def pack_bits(flags, words):
    out = np.zeros(words, np.uint32)
    for j in np.nonzero(flags)[0]:
        out[j >> 5] |= np.uint32(1 << (j & 31))
    return out


def events_of(counts, min_inliers):
    """The iterations at which iterate() would return: n_k > min_inliers and n_k >= every earlier count (mnBestInliers starts at 0)."""
    best, ev = 0, []
    for k, n in enumerate(counts):
        if n >= best:
            best = n
            if n > min_inliers:
                ev.append(k)
    return ev


# ------------------------------------------------------------------------------------------------ the whole call, one candidate
def run(s):
    """Every output row of orbfe_enqueue_sim3_ransac_batch for one candidate scene."""
    max_its, max_pairs = s["max_its"], s["max_pairs"]
    words = (max_pairs + 31) // 32
    out = dict(status=0, n_corr=0, n_its=0, corr=np.full((max_pairs, 2), -1, np.int32), sets=np.full((max_its, 3), -1, np.int32),
               hyp=np.zeros(max_its, HYP_DTYPE), bits=np.zeros((max_its, words), np.uint32), events=np.full(max_its, -1, np.int32), n_events=0)
    n1, n2 = len(s["keys1"]), len(s["keys2"])
    if n2 > s["max_kf_n"] or len(s["pairs"]) > max_pairs:      # what the device refuses in a record (kf1 is checked by the call itself)
        out["status"] = ERR_INVALID
        return out
    status, corr, tab = filter_pairs(s)
    N = len(corr)
    out["status"], out["n_corr"] = status, N
    out["corr"][:N] = corr
    n_its = min(int(s["its_for_n"][N]), max_its)
    out["n_its"] = n_its
    for k in range(n_its):
        ids = draw_set(s["draws"][k], N)
        P1 = tab["X1"][list(ids)].T.copy()
        P2 = tab["X2"][list(ids)].T.copy()
        R, t, sc, sR, sRinv, tinv = compute_sim3(P1, P2, s["fix_scale"])
        flags, _, _ = check_inliers(tab, sR, t, sRinv, tinv, s["cam"])
        out["sets"][k] = ids
        h = out["hyp"][k]
        h["n_inliers"], h["s12"], h["R12"], h["t12"] = int(flags.sum()), stored(sc), stored(R.reshape(9)), stored(t)
        out["bits"][k] = pack_bits(flags, words)
    ev = events_of(out["hyp"]["n_inliers"][:n_its], s["min_inliers"])
    out["n_events"] = len(ev)
    out["events"][:len(ev)] = ev
    out["table"] = tab
    return out


def select_rows(out, k, n1, valid1, valid2):
    """orbfe_enqueue_sim3_ransac_select: (prior12, valid1_round, valid2_round) of hypothesis k (src/LoopClosing.cc:349-354 and the
    !vbAlreadyMatched terms of src/ORBmatcher.cc:1125-1152)."""
    prior = np.full(n1, -1, np.int32)
    v2 = (np.asarray(valid2) != 0).astype(np.int32)
    for j in range(out["n_corr"]):
        if out["bits"][k][j >> 5] >> np.uint32(j & 31) & np.uint32(1):
            i1, i2 = out["corr"][j]
            prior[i1] = i2
            v2[i2] = 0
    v1 = ((np.asarray(valid1) != 0) & (prior < 0)).astype(np.int32)
    return prior, v1, v2


# ------------------------------------------------------------------------------------------------ the float64 yardstick
def reference_errors(tab, ids, fix_scale, cam):
    """ComputeSim3 + CheckInliers in float64 as the reference is shaped: eigh, atan2 and the angle-axis of :275-285, Rodrigues.  Returns
    (err1, err2, R, t, s) in float64, on the table's float32 points."""
    X1, X2 = tab["X1"].astype(f64), tab["X2"].astype(f64)
    P1, P2 = X1[list(ids)].T, X2[list(ids)].T
    O1, O2 = P1.sum(1) / 3, P2.sum(1) / 3
    Pr1, Pr2 = P1 - O1[:, None], P2 - O2[:, None]
    M = Pr2 @ Pr1.T
    N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                  [0, M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                  [0, 0, -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                  [0, 0, 0, -M[0, 0] - M[1, 1] + M[2, 2]]])
    N = N + np.triu(N, 1).T
    w, v = np.linalg.eigh(N)
    q = v[:, np.argmax(w)]
    vec = q[1:4]
    with np.errstate(all="ignore"):
        ang = math.atan2(np.linalg.norm(vec), q[0])
        rv = 2 * ang * vec / np.linalg.norm(vec)
        th = np.linalg.norm(rv)
        k = rv / th
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R = math.cos(th) * np.eye(3) + (1 - math.cos(th)) * np.outer(k, k) + math.sin(th) * K     # cv::Rodrigues
        P3 = R @ Pr2
        s = 1.0 if fix_scale else float((Pr1 * P3).sum() / (P3 * P3).sum())
        t = O1 - s * R @ O2
        sRi = (1.0 / s) * R.T
        ti = -sRi @ t
        fx, fy, cx, cy = cam

        def proj(X, A, b):
            P = X @ A.T + b
            return np.stack([fx * P[:, 0] / P[:, 2] + cx, fy * P[:, 1] / P[:, 2] + cy], axis=1)
        p1, p2 = proj(X1, np.eye(3), 0), proj(X2, np.eye(3), 0)
        e1 = ((p1 - proj(X2, s * R, t)) ** 2).sum(1)
        e2 = ((proj(X1, sRi, ti) - p2) ** 2).sum(1)
    return e1, e2, R, t, s


# ------------------------------------------------------------------------------------------------ Sim3Solver::iterate, literally
class Solver:
    """src/Sim3Solver.cc:141-208 with ComputeSim3 + CheckInliers replaced by a lookup of hypothesis mnIterations - 1's stored results
    (counts[k], and whatever `payload` holds).  N, min_inliers and max_its are the members after SetRansacParameters."""

    def __init__(self, N, counts, min_inliers, max_its):
        self.N, self.counts, self.min_inliers, self.max_its = N, counts, min_inliers, max_its
        self.mnIterations, self.mnBestInliers, self.best = 0, 0, -1

    def iterate(self, nIterations):
        """Returns (k or -1, bNoMore, nInliers): k is the hypothesis whose T12 the reference would return."""
        bNoMore, nInliers = False, 0
        if self.N < self.min_inliers:
            return -1, True, 0
        cur = 0
        while self.mnIterations < self.max_its and cur < nIterations:
            cur += 1
            self.mnIterations += 1
            n = int(self.counts[self.mnIterations - 1])
            if n >= self.mnBestInliers:
                self.mnBestInliers, self.best = n, self.mnIterations - 1
                if n > self.min_inliers:
                    return self.best, bNoMore, n
        if self.mnIterations >= self.max_its:
            bNoMore = True
        return -1, bNoMore, nInliers
