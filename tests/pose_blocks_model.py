"""Float64 (and, for the evaluation pass, extended precision) references of the device blocks of
orbslam2_amd/csrc/orbfe_pose_blocks.hpp, for tests/test_pose_blocks.py.  Plain numpy / scipy, no GPU, no oracle: the CPU
tests of test_pose_blocks.py check each of them against the oracle's hooks before a GPU sees them.

Conventions: a pose is seven doubles (x, y, z, w, tx, ty, tz) like the kernel's Se3; Hu is the kernel's packed system,
21 upper-triangle entries row-major followed by b[6].
"""
import math

import numpy as np

DBL_MIN = np.finfo(np.float64).tiny
DELTA_MONO = float(np.float32(math.sqrt(5.991)))      # src/Optimizer.cc:317-318: const float deltaMono = sqrt(5.991)
DELTA_STEREO = float(np.float32(math.sqrt(7.815)))


# ---------------------------------------------------------------- quaternions and SE3

def rot(rv):
    """Rodrigues, float64."""
    rv = np.asarray(rv, np.float64)
    th = np.linalg.norm(rv)
    if th == 0:
        return np.eye(3)
    k = rv / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def quat_branch(m):
    """Which branch Eigen's Quaternion(Matrix3) takes: 'trace' or the index of the largest diagonal entry, the lower index
    on ties (the strict '>' tests of quaternionbase_assign_impl)."""
    if m[0][0] + m[1][1] + m[2][2] > 0.0:
        return "trace"
    i = 0
    if m[1][1] > m[0][0]:
        i = 1
    if m[2][2] > m[i][i]:
        i = 2
    return i


def quat_from_matrix(m):
    """(x, y, z, w) of Eigen's Quaternion(Matrix3), then SE3Quat::normalizeRotation (w >= 0, unit).  Returns (q, branch)."""
    m = np.asarray(m, np.float64)
    br = quat_branch(m)
    c = np.zeros(4)
    if br == "trace":
        t = math.sqrt(m[0][0] + m[1][1] + m[2][2] + 1.0)
        c[3] = 0.5 * t
        t = 0.5 / t
        c[0] = (m[2][1] - m[1][2]) * t
        c[1] = (m[0][2] - m[2][0]) * t
        c[2] = (m[1][0] - m[0][1]) * t
    else:
        i = br
        j, k = (i + 1) % 3, (i + 2) % 3
        t = math.sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0)
        c[i] = 0.5 * t
        t = 0.5 / t
        c[3] = (m[k][j] - m[j][k]) * t
        c[j] = (m[j][i] + m[i][j]) * t
        c[k] = (m[k][i] + m[i][k]) * t
    if c[3] < 0:
        c = -c
    return c / math.sqrt(float(c @ c)), br


def quat_to_matrix(q):
    x, y, z, w = (float(v) for v in q[:4])
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def pose_to_matrix(p):
    T = np.eye(4)
    T[:3, :3] = quat_to_matrix(p[:4])
    T[:3, 3] = p[4:7]
    return T


def pose_from_cv(T):
    """Converter::toSE3Quat on a float32 4x4.  Returns (pose[7], branch)."""
    T = np.asarray(T, np.float32).reshape(4, 4).astype(np.float64)
    q, br = quat_from_matrix(T[:3, :3])
    return np.concatenate([q, T[:3, 3]]), br


def pose_to_cv(p):
    """Converter::toCvMat(SE3Quat): the float32 4x4."""
    return pose_to_matrix(p).astype(np.float32)


def skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)


def se3_exp_matrix(u):
    """expm of the 4x4 twist (omega first, upsilon second, as SE3Quat::exp takes them)."""
    from scipy.linalg import expm
    A = np.zeros((4, 4))
    A[:3, :3] = skew(u[:3])
    A[:3, 3] = u[3:6]
    return expm(A)


def se3_exp_small(u):
    """What SE3Quat::exp does below theta = 1e-5: R = V = I + Omega + Omega^2 (se3quat.h:232-238), the quaternion of that R
    (not orthonormal: the normalisation takes care), t = V upsilon.  Returns pose[7]."""
    u = np.asarray(u, np.float64)
    O = skew(u[:3])
    R = np.eye(3) + O + O @ O
    q, _ = quat_from_matrix(R)
    return np.concatenate([q, R @ u[3:6]])


def se3_mul(a, b):
    """SE3Quat::operator*: Hamilton product, normalizeRotation, t = a.t + a.R b.t.  Returns pose[7]."""
    ax, ay, az, aw = a[:4]
    bx, by, bz, bw = b[:4]
    q = np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                  aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])
    if q[3] < 0:
        q = -q
    q = q / math.sqrt(float(q @ q))
    return np.concatenate([q, np.asarray(a[4:7]) + quat_to_matrix(a) @ np.asarray(b[4:7])])


# ---------------------------------------------------------------- LDLT with diagonal pivoting

def pack_system(H, b):
    H = np.asarray(H, np.float64)
    return np.concatenate([H[np.triu_indices(6)], np.asarray(b, np.float64)])


def ldlt_solve(H, b, lam=0.0):
    """Eigen::LDLT as LinearSolverDense uses it, on H + lam I: at step k the largest |diagonal| of the tail is exchanged
    into place (first one wins), a pivot with |d| <= DBL_MIN gives a zero column and a zero in the D^-1 step.
    Returns (x or None when the factor is not positive, positive, [(k, pivot)] for the six steps)."""
    A = np.array(H, np.float64).reshape(6, 6).copy()
    A[np.diag_indices(6)] += lam
    y = np.array(b, np.float64).copy()
    piv = []
    positive = True
    with np.errstate(all="ignore"):
        for k in range(6):
            p, big = k, abs(A[k, k])
            for i in range(k + 1, 6):
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
            for i in range(k + 1, 6):
                s = A[i, k]
                for j in range(k):
                    s -= A[i, j] * A[k, j] * A[j, j]
                A[i, k] = s / d if abs(d) > DBL_MIN else 0.0
        if not positive:
            return None, False, piv
        for i in range(6):
            for j in range(i):
                y[i] -= A[i, j] * y[j]
        for i in range(6):
            y[i] = y[i] / A[i, i] if abs(A[i, i]) > DBL_MIN else 0.0
        for i in range(5, -1, -1):
            for j in range(i + 1, 6):
                y[i] -= A[j, i] * y[j]
        for k, p in reversed(piv):
            if p != k:
                y[[k, p]] = y[[p, k]]
    return y, True, piv


def exchanges(piv):
    return {(k, p) for k, p in piv if p != k}


def pivot_matrix(K, C, seed):
    """A symmetric, strictly diagonally dominant (hence positive definite) matrix with dense off-diagonals whose diagonal is
    ordered so that steps 0..K-1 keep their place and step K exchanges with C, and a dense right-hand side.  (The pivot
    search looks at the original diagonal: the factorisation is left-looking, the tail of the diagonal is not updated.)"""
    rng = np.random.default_rng(seed)
    d = np.empty(6)
    rest = 200.0
    for i in range(6):
        if i < K:
            d[i] = 600.0 - 40.0 * i
        elif i == C:
            d[i] = 300.0
        else:
            d[i] = rest
            rest -= 25.0
    H = rng.uniform(-8, 8, (6, 6))
    H = (H + H.T) / 2
    H[np.diag_indices(6)] = d + rng.uniform(0, 1, 6)
    return H, rng.uniform(-50, 50, 6)


# ---------------------------------------------------------------- the evaluation pass

def eval_reference(keys, u_right, has_point, Xw, outlier, inv_sigma2, pose, cam, robust):
    """s_tot[0..28] of eval_pass over the active edges (map point, not marked outlier) at `pose`: the 21 upper entries of
    J^T W J, the 6 of -J^T W e, the robust chi2 and the number of active edges.

    Per-edge quantities are formed in extended precision (numpy longdouble) from the float32 inputs and the float64 pose,
    with the two roundings the reference arithmetic itself makes kept: the stereo edge's `const float invz` and the float
    Huber delta.  Each per-edge addend is then rounded to float64 and the totals are math.fsum's of them, so the reference
    is exact to a small fraction of the bound it is used with.

    Returns (tot[29], mag[29]): mag[k] is the sum of the magnitudes the roundings of total k are relative to -- see
    test_pose_blocks.eval_bound."""
    LD = np.longdouble
    fx, fy, cx, cy, bf = (LD(v) for v in cam)
    qv = np.array([LD(float(v)) for v in pose[:3]])
    qw = LD(float(pose[3]))
    t = np.array([LD(float(v)) for v in pose[4:7]])
    adds = [[] for _ in range(29)]
    mags = [[] for _ in range(29)]
    for i in range(len(keys)):
        if not has_point[i] or outlier[i]:
            continue
        X = np.array([LD(float(v)) for v in Xw[i]])
        uv = 2 * np.cross(qv, X)                      # Eigen's _transformVector, the formula the kernel uses
        p = X + qw * uv + np.cross(qv, uv) + t
        stereo = not (u_right[i] < 0)
        info = LD(float(inv_sigma2[keys["octave"][i]]))
        invz = LD(1) / p[2]
        iz = LD(float(np.float32(np.float64(invz)))) if stereo else invz
        proj = [p[0] * iz * fx + cx, p[1] * iz * fy + cy]
        obs = [LD(float(keys["x"][i])), LD(float(keys["y"][i]))]
        if stereo:
            proj.append(proj[0] - bf * iz)
            obs.append(LD(float(u_right[i])))
        D = len(proj)
        err = [obs[d] - proj[d] for d in range(D)]
        chi = sum(info * e * e for e in err)
        # first-order conditioning of chi2: its error is 2 info |err| (|obs| + |proj|) roundings, not chi2 roundings
        chi_mag = 2 * sum(info * abs(err[d]) * (abs(obs[d]) + abs(proj[d])) for d in range(D))
        w, rho0, rho_mag, kap = LD(1), chi, chi_mag, LD(0)
        if robust:
            delta = LD(DELTA_STEREO if stereo else DELTA_MONO)
            dsqr = LD(float(np.float64(delta) * np.float64(delta)))  # the kernel squares the double
            if chi > dsqr:
                s = np.sqrt(chi)
                rho0 = 2 * s * delta - dsqr
                w = delta / s
                kap = chi_mag / chi / 2          # relative error of sqrt(chi), in units of one rounding
                rho_mag = 2 * s * delta * (1 + kap) + dsqr
        x, y, iz2 = p[0], p[1], invz * invz
        J = [[x * y * iz2 * fx, -(1 + x * x * iz2) * fx, y * invz * fx, -invz * fx, LD(0), x * iz2 * fx],
             [(1 + y * y * iz2) * fy, -x * y * iz2 * fy, -x * invz * fy, LD(0), -invz * fy, y * iz2 * fy]]
        if stereo:
            J.append([J[0][0] - bf * y * iz2, J[0][1] + bf * x * iz2, J[0][2], J[0][3], LD(0), J[0][5] - bf * iz2])
        wi = w * info
        k = 0
        for a in range(6):
            for b in range(a, 6):
                prods = [J[d][a] * wi * J[d][b] for d in range(D)]
                adds[k].append(float(sum(prods)))
                mags[k].append(float(sum(abs(v) for v in prods) * (1 + kap)))
                k += 1
        for a in range(6):
            adds[21 + a].append(float(-sum(J[d][a] * wi * err[d] for d in range(D))))
            mags[21 + a].append(float(sum(abs(J[d][a]) * wi * (abs(obs[d]) + abs(proj[d]) + kap * abs(err[d])) for d in range(D))))
        adds[27].append(float(rho0))
        mags[27].append(float(rho_mag))
        adds[28].append(1.0)
        mags[28].append(0.0)   # a count: exact
    return np.array([math.fsum(a) for a in adds]), np.array([math.fsum(m) for m in mags])

