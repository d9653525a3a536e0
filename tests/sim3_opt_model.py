"""Float64 model of orbfe_enqueue_optimize_sim3 (include/orbfe.h): Optimizer::OptimizeSim3 (reference src/Optimizer.cc:1090-1285) restated
on keypoint slots, with g2o's Sim3 algebra (Thirdparty/g2o/g2o/types/sim3.h), the two projection edges
(types_seven_dof_expmap.h:130-171), BaseBinaryEdge's NUMERIC Jacobian (core/base_binary_edge.hpp:131-204: central differences, delta 1e-9,
through oplus), the Huber quadratic form (:91-113), Eigen's LDLT with diagonal pivoting and OptimizationAlgorithmLevenberg /
SparseOptimizer::optimize.  It is the reference of tests/test_sim3_opt_model.py (which proves it), tests/test_sim3_blocks.py and
tests/test_sim3_opt_device.py (which compare the kernels with it).

Edge-sequential: numpy arrays run ACROSS the correspondences only (the error of every edge under one Sim3), never along a sum -- the
normal equations and the robust chi2 are Python loops in g2o's edge order (e12 of the first correspondence, its e21, the next e12 ...).
sin, cos and exp are math's, on scalars.  A Sim3 is (q, t, s): q = (x, y, z, w) as g2o keeps it, never normalised.
"""
import math

import numpy as np

ERR_INVALID = -1
DEFAULT_PARAMS = (5, 10, 5, 10)   # iterations, more_iterations_outliers, more_iterations_clean, min_inliers (src/Optimizer.cc:60-70)
NUM_DELTA = 1e-9                  # base_binary_edge.hpp:147
DBL_MIN = np.finfo(np.float64).tiny
DBL_MAX = np.finfo(np.float64).max


# ---------------------------------------------------------------- Sim3 algebra
def quat_of_matrix(m):
    """Eigen's Quaternion(Matrix3) as (x, y, z, w), NOT normalised; the lower index wins a tie of the diagonal."""
    m = [[float(m[i][j]) for j in range(3)] for i in range(3)]
    c = [0.0] * 4
    t = m[0][0] + m[1][1] + m[2][2]
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        c[3] = 0.5 * t
        t = 0.5 / t
        c[0] = (m[2][1] - m[1][2]) * t
        c[1] = (m[0][2] - m[2][0]) * t
        c[2] = (m[1][0] - m[0][1]) * t
    else:
        i = 0
        if m[1][1] > m[0][0]:
            i = 1
        if m[2][2] > m[i][i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = math.sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0)
        c[i] = 0.5 * t
        t = 0.5 / t
        c[3] = (m[k][j] - m[j][k]) * t
        c[j] = (m[j][i] + m[i][j]) * t
        c[k] = (m[k][i] + m[i][k]) * t
    return tuple(c)


def sim3(R, t, s):
    """Sim3(Matrix3d, Vector3d, double)."""
    return (quat_of_matrix(R), tuple(float(v) for v in t), float(s))


def rotate(q, vx, vy, vz):
    """Eigen's Quaternion * Vector3 (_transformVector: v + w uv + q x uv with uv = 2 q x v); scalars or arrays."""
    x, y, z, w = q
    ux, uy, uz = y * vz - z * vy, z * vx - x * vz, x * vy - y * vx
    ux, uy, uz = ux + ux, uy + uy, uz + uz
    cx, cy, cz = y * uz - z * uy, z * ux - x * uz, x * uy - y * ux
    return vx + w * ux + cx, vy + w * uy + cy, vz + w * uz + cz


def sim3_map(S, px, py, pz):
    q, t, s = S
    rx, ry, rz = rotate(q, px, py, pz)
    return s * rx + t[0], s * ry + t[1], s * rz + t[2]


def sim3_mul(a, b):
    (ax, ay, az, aw), at, as_ = a
    (bx, by, bz, bw), bt, bs = b
    rx, ry, rz = rotate(a[0], bt[0], bt[1], bt[2])
    q = (aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
         aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz)
    return (q, (as_ * rx + at[0], as_ * ry + at[1], as_ * rz + at[2]), as_ * bs)


def sim3_inverse(a):
    (x, y, z, w), t, s = a
    qc = (-x, -y, -z, w)
    k = -1.0 / s
    return (qc, rotate(qc, k * t[0], k * t[1], k * t[2]), 1.0 / s)


def exp_branch(u):
    sigma, theta = float(u[6]), math.sqrt(float(u[0]) ** 2 + float(u[1]) ** 2 + float(u[2]) ** 2)
    return (abs(sigma) < 0.00001, theta < 0.00001)


def sim3_exp(u):
    """Sim3(Vector7d), all four (|sigma| < 1e-5, theta < 1e-5) branches as written."""
    u = [float(v) for v in u]
    om, ups, sigma = u[0:3], u[3:6], u[6]
    theta = math.sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2])
    O = [[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]]
    O2 = [[sum(O[i][k] * O[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
    s = math.exp(sigma)
    eps = 0.00001
    if theta < eps:
        ra, rb = 1.0, 1.0                                  # R = I + Omega + Omega^2: not orthonormal
    else:
        ra, rb = math.sin(theta) / theta, (1 - math.cos(theta)) / (theta * theta)
    if abs(sigma) < eps:
        C = 1.0
        if theta < eps:
            A, B = 1. / 2., 1. / 6.
        else:
            theta2 = theta * theta
            A = (1 - math.cos(theta)) / theta2
            B = (theta - math.sin(theta)) / (theta2 * theta)
    else:
        C = (s - 1) / sigma
        if theta < eps:
            sigma2 = sigma * sigma
            A = ((sigma - 1) * s + 1) / sigma2
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
        else:
            a, b = s * math.sin(theta), s * math.cos(theta)
            theta2, sigma2 = theta * theta, sigma * sigma
            c = theta2 + sigma2
            A = (a * sigma + (1 - b) * theta) / (theta * c)
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2
    I = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    R = [[I[i][j] + ra * O[i][j] + rb * O2[i][j] for j in range(3)] for i in range(3)]
    t = []
    for i in range(3):
        acc = 0.0
        for j in range(3):
            acc += (A * O[i][j] + B * O2[i][j] + C * I[i][j]) * ups[j]
        t.append(acc)
    return (quat_of_matrix(R), tuple(t), s)


def oplus(update, fix_scale, est):
    """VertexSim3Expmap::oplusImpl."""
    u = [float(v) for v in update]
    if fix_scale:
        u[6] = 0.0
    return sim3_mul(sim3_exp(u), est)


def quat_matrix(q):
    """Eigen's toRotationMatrix of (x, y, z, w) -- of any norm, as the tests compare rotations."""
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def sim3_matrix(S):
    """The 4 x 4 similarity [[s R, t], [0, 1]]."""
    M = np.eye(4)
    M[:3, :3] = S[2] * quat_matrix(S[0])
    M[:3, 3] = S[1]
    return M


def pack(S):
    return np.array(list(S[0]) + list(S[1]) + [S[2]], np.float64)


def unpack(v):
    v = [float(x) for x in v]
    return (tuple(v[0:4]), tuple(v[4:7]), v[7])


# ---------------------------------------------------------------- edges
def edge_error(S, cam, P, obs):
    """obs - cam_map(project(S.map(P))) for the rows of P [N][3] and obs [N][2]: (e0[N], e1[N])."""
    fx, fy, cx, cy = cam
    px, py, pz = sim3_map(S, P[:, 0], P[:, 1], P[:, 2])
    return obs[:, 0] - (px / pz * fx + cx), obs[:, 1] - (py / pz * fy + cy)


def pass_sims(est, fix_scale):
    """The 15 Sim3s of one linearisation, each with its inverse: [2 d] = oplus(+delta e_d), [2 d + 1] = oplus(-delta e_d), [14] = est."""
    out = []
    for d in range(7):
        for sgn in (1.0, -1.0):
            u = [0.0] * 7
            u[d] = sgn * NUM_DELTA
            S = oplus(u, fix_scale, est)
            out.append((S, sim3_inverse(S)))
    out.append((est, sim3_inverse(est)))
    return out


def huber(e2, delta):
    dsqr = delta * delta
    if e2 <= dsqr:
        return e2, 1.0
    sq = math.sqrt(e2)
    return 2 * sq * delta - dsqr, delta / sq


class Table:
    """The correspondences of one call in ascending slot of KF1: P1c, P2c [N][3], obs1, obs2 [N][2], info1, info2 [N] (float64 copies
    of the floats the reference holds), slot [N], active [N] (False once removed)."""

    def __init__(self, P1, P2, obs1, obs2, info1, info2, slot):
        self.P1, self.P2 = np.asarray(P1, np.float64).reshape(-1, 3), np.asarray(P2, np.float64).reshape(-1, 3)
        self.obs1, self.obs2 = np.asarray(obs1, np.float64).reshape(-1, 2), np.asarray(obs2, np.float64).reshape(-1, 2)
        self.info1, self.info2 = np.asarray(info1, np.float64).reshape(-1), np.asarray(info2, np.float64).reshape(-1)
        self.slot = np.asarray(slot, np.int64).reshape(-1)
        self.active = np.ones(len(self.slot), bool)

    def __len__(self):
        return len(self.slot)


def edge_chi2(T, S, cam):
    """(chi2 of e12 [N], chi2 of e21 [N]) at S: BaseEdge::chi2 = e . (information e)."""
    a0, a1 = edge_error(S, cam, T.P2, T.obs1)
    b0, b1 = edge_error(sim3_inverse(S), cam, T.P1, T.obs2)
    return a0 * (T.info1 * a0) + a1 * (T.info1 * a1), b0 * (T.info2 * b0) + b1 * (T.info2 * b1)


def evaluate(T, est, fix_scale, cam, delta):
    """One evaluation pass at `est` over the active correspondences.  Returns (H[7][7], b[7], robust chi2, #active, J12[N][2][7],
    J21[N][2][7])."""
    n = len(T)
    sims = pass_sims(est, fix_scale)
    scalar = 1.0 / (2 * NUM_DELTA)
    J12, J21 = np.zeros((n, 2, 7)), np.zeros((n, 2, 7))
    with np.errstate(all="ignore"):
        for d in range(7):
            p0, p1 = edge_error(sims[2 * d][0], cam, T.P2, T.obs1)
            m0, m1 = edge_error(sims[2 * d + 1][0], cam, T.P2, T.obs1)
            J12[:, 0, d], J12[:, 1, d] = scalar * (p0 - m0), scalar * (p1 - m1)
            p0, p1 = edge_error(sims[2 * d][1], cam, T.P1, T.obs2)
            m0, m1 = edge_error(sims[2 * d + 1][1], cam, T.P1, T.obs2)
            J21[:, 0, d], J21[:, 1, d] = scalar * (p0 - m0), scalar * (p1 - m1)
        e12 = np.stack(edge_error(sims[14][0], cam, T.P2, T.obs1), 1)
        e21 = np.stack(edge_error(sims[14][1], cam, T.P1, T.obs2), 1)
        H, b, chi, cnt = np.zeros((7, 7)), np.zeros(7), 0.0, 0
        for k in range(n):
            if not T.active[k]:
                continue
            cnt += 1
            for J, e, info in ((J12[k], e12[k], float(T.info1[k])), (J21[k], e21[k], float(T.info2[k]))):
                e0, e1 = float(e[0]), float(e[1])
                c2 = e0 * (info * e0) + e1 * (info * e1)
                rho0, rho1 = huber(c2, delta)
                chi += rho0
                wi = info * rho1
                or0, or1 = -(info * e0) * rho1, -(info * e1) * rho1
                H += np.outer(J[0] * wi, J[0]) + np.outer(J[1] * wi, J[1])
                b += J[0] * or0 + J[1] * or1
    return H, b, chi, cnt, J12, J21


# ---------------------------------------------------------------- LDLT with diagonal pivoting, any dimension
def ldlt_solve(H, b, lam=0.0):
    """Eigen::LDLT as LinearSolverDense uses it, on H + lam I (tests/pose_blocks_model.ldlt_solve for any dimension).  Returns
    (x or None when the factor is not positive, positive, [(k, pivot)])."""
    n = len(b)
    A = np.array(H, np.float64).reshape(n, n).copy()
    A[np.diag_indices(n)] += lam
    y = np.array(b, np.float64).copy()
    piv, positive = [], True
    with np.errstate(all="ignore"):
        for k in range(n):
            p, big = k, abs(A[k, k])
            for i in range(k + 1, n):
                if abs(A[i, i]) > big:
                    big, p = abs(A[i, i]), i
            piv.append((k, p))
            if p != k:
                A[[k, p], :] = A[[p, k], :]
                A[:, [k, p]] = A[:, [p, k]]
                y[[k, p]] = y[[p, k]]
            d = A[k, k]
            for j in range(k):
                d -= A[k, j] * A[k, j] * A[j, j]
            A[k, k] = d
            if d < 0:
                positive = False
            for i in range(k + 1, n):
                s = A[i, k]
                for j in range(k):
                    s -= A[i, j] * A[k, j] * A[j, j]
                A[i, k] = s / d if abs(d) > DBL_MIN else 0.0
        if not positive:
            return None, False, piv
        for i in range(n):
            for j in range(i):
                y[i] -= A[i, j] * y[j]
        for i in range(n):
            y[i] = y[i] / A[i, i] if abs(A[i, i]) > DBL_MIN else 0.0
        for i in range(n - 1, -1, -1):
            for j in range(i + 1, n):
                y[i] -= A[j, i] * y[j]
        for k, p in reversed(piv):
            if p != k:
                y[[k, p]] = y[[p, k]]
    return y, True, piv


# ---------------------------------------------------------------- Levenberg
def optimize(T, est, iterations, fix_scale, cam, delta):
    """SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg.  Returns (estimate, last evaluated estimate,
    iterations run, trials run)."""
    last_eval = est
    H, b, chi, cnt, _, _ = evaluate(T, est, fix_scale, cam, delta)
    iters = trials = 0
    if cnt == 0:
        return est, last_eval, 0, 0
    current_chi = chi
    lam, ni, lm_bad = -1.0, 2.0, 0
    x = np.zeros(7)
    for it in range(iterations):
        iters += 1
        last_eval = est
        ini_chi = current_chi
        if it == 0:
            lam = 1e-5 * max(abs(float(H[j, j])) for j in range(7))
            ni, lm_bad = 2.0, 0
        rho, qmax = 0.0, 0
        while True:
            xs, ok2, _ = ldlt_solve(H, b, lam)
            if ok2:
                x = xs
            scale = 0.0
            for j in range(7):
                scale += x[j] * (lam * x[j] + b[j])
            scale += 1e-3
            trial = oplus(x, fix_scale, est)
            Ht, bt, chit, _, _, _ = evaluate(T, trial, fix_scale, cam, delta)
            trials += 1
            last_eval = trial
            temp_chi = chit if ok2 else DBL_MAX
            rho = (current_chi - temp_chi) / scale
            if rho > 0 and math.isfinite(temp_chi):
                alpha = 1.0 - (2 * rho - 1) ** 3
                alpha = min(alpha, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni = 2.0
                current_chi = temp_chi
                est, H, b = trial, Ht, bt
            else:
                lam *= ni
                ni *= 2
            qmax += 1
            if not (rho < 0 and qmax < 10):
                break
        if qmax == 10 or rho == 0:
            break
        lm_bad = lm_bad + 1 if (ini_chi - current_chi) * 1e3 < ini_chi else 0
        if lm_bad >= 3:
            break
    return est, last_eval, iters, trials


# ---------------------------------------------------------------- the call
def cv_point(T34, X):
    """R * X + t as a float cv::Mat expression: per row a double sum in index order plus t, rounded once (the `+ C` form)."""
    out = np.zeros(3, np.float32)
    for r in range(3):
        s = 0.0
        for k in range(3):
            s += float(T34[r, k]) * float(X[k])
        out[r] = np.float32(s + float(T34[r, 3]))
    return out


def build_table(keys1, T1w, pos1, valid1, keys2, T2w, pos2, valid2, prior12, match12, inv_sigma2, nlevels):
    """Section 1 of the contract.  Returns (Table, merged match12, status)."""
    n1, n2 = len(keys1), len(keys2)
    T1 = np.asarray(T1w, np.float32).reshape(-1)[:12].reshape(3, 4)
    T2 = np.asarray(T2w, np.float32).reshape(-1)[:12].reshape(3, 4)
    out = np.asarray(match12, np.int32).copy()
    status = 0
    rows = []
    for i in range(n1):
        m = int(prior12[i]) if prior12 is not None and prior12[i] >= 0 else int(out[i])
        if m == -1:
            out[i] = -1
            continue
        ok = 0 <= m < n2
        if ok:
            o1, o2 = int(keys1["octave"][i]), int(keys2["octave"][m])
            ok = 0 <= o1 < nlevels and 0 <= o2 < nlevels
        if not ok:
            status = ERR_INVALID
            out[i] = -1
            continue
        out[i] = m
        if not valid1[i] or not valid2[m]:
            continue
        rows.append((cv_point(T1, pos1[i]), cv_point(T2, pos2[m]), (keys1["x"][i], keys1["y"][i]), (keys2["x"][m], keys2["y"][m]),
                     inv_sigma2[o1], inv_sigma2[o2], i))
    cols = list(zip(*rows)) if rows else [[], [], [], [], [], [], []]
    return Table(*cols), out, status


def optimize_sim3(keys1, T1w, pos1, valid1, keys2, T2w, pos2, valid2, s12, R12, t12, th2, fix_scale, match12, cam, inv_sigma2, nlevels=8,
                  prior12=None, params=None):
    """The whole call.  Returns a dict: S12 [8] (qx qy qz qw tx ty tz s), match12, n_inliers, status, and for the tests n_corr, slots,
    chi_first / chi_second (chi2 of (e12, e21) per correspondence at the two classifications; None where it did not happen),
    active_second, iterations and trials of both optimize() calls."""
    iterations, more_out, more_clean, min_inliers = params or DEFAULT_PARAMS
    th2 = float(np.float32(th2))
    delta = float(np.float32(math.sqrt(th2)))
    cam = tuple(float(np.float32(v)) for v in cam)
    T, out, status = build_table(keys1, T1w, pos1, valid1, keys2, T2w, pos2, valid2, prior12, match12, np.asarray(inv_sigma2, np.float32), nlevels)
    S_in = sim3(np.asarray(R12, np.float32).reshape(3, 3).astype(np.float64), np.asarray(t12, np.float32).astype(np.float64), float(np.float32(s12)))
    res = dict(S12=pack(S_in), match12=out, n_inliers=0, status=status, n_corr=len(T), slots=T.slot.copy(), chi_first=None, chi_second=None,
               active_second=None, iterations=[0, 0], trials=[0, 0], table=T)
    if len(T) == 0:
        return res
    est, last_eval, it, tr = optimize(T, S_in, iterations, bool(fix_scale), cam, delta)
    res["iterations"][0], res["trials"][0] = it, tr
    c12, c21 = edge_chi2(T, last_eval, cam)
    res["chi_first"] = np.stack([c12, c21], 1)
    bad = (c12 > th2) | (c21 > th2)
    out[T.slot[bad]] = -1
    T.active &= ~bad
    n_bad = int(bad.sum())
    if len(T) - n_bad < min_inliers:
        return res
    est, last_eval, it, tr = optimize(T, est, more_out if n_bad > 0 else more_clean, bool(fix_scale), cam, delta)
    res["iterations"][1], res["trials"][1] = it, tr
    c12, c21 = edge_chi2(T, last_eval, cam)
    res["chi_second"] = np.stack([c12, c21], 1)
    res["active_second"] = T.active.copy()
    bad2 = T.active & ((c12 > th2) | (c21 > th2))
    out[T.slot[bad2]] = -1
    res["n_inliers"] = int((T.active & ~bad2).sum())
    res["S12"] = pack(est)
    return res
