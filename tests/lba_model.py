"""Float64 model of orbfe_enqueue_local_bundle_adjustment (Optimizer::LocalBundleAdjustment, reference src/Optimizer.cc:566-822, after
the graph walk of :499-548 has become roles and observation lists).  Plain numpy: per-edge arithmetic runs across the edges, every sum
over edges is np.add.at or a Python loop in edge order, the Schur complement is written as BlockSolver<6,3>::solve writes it
(core/block_solver.hpp:353-486) and the reduced system goes through a dense LDLT without pivoting that fails on an exactly zero pivot
(LinearSolverEigen's SimplicialLDLT without its fill-reducing ordering).  tests/test_lba_model.py proves this module on the CPU;
tests/test_lba_device.py compares the device with it.

Conventions: a pose is seven doubles (x, y, z, w, tx, ty, tz) as in tests/pose_blocks_model.py; an edge is an entry j of the
observation arrays; `quirks` names the reference behaviours that the quirk tests switch off one at a time.
"""
import math

import numpy as np

from tests import cvmat_model as CV
from tests import pose_blocks_model as PB

ERR_INVALID, ERR_CAPACITY = -1, -4
SKIP, LOCAL, LOCAL_HELD, FIXED = 0, 1, 2, 3
CODE_LEVEL1, CODE_ERASE, CODE_SKIPPED, CODE_FAULTY = 1, 2, 4, 8
DELTA_MONO, DELTA_STEREO = PB.DELTA_MONO, PB.DELTA_STEREO
CHI2_MONO, CHI2_STEREO = 5.991, 7.815
DBL_MAX = np.finfo(np.float64).max
ALL_QUIRKS = frozenset(("stale_chi2", "orphans", "held_rewrite", "fixed_bits"))


# ---------------------------------------------------------------- SE3

def se3_exp(u):
    """SE3Quat::exp (types/se3quat.h:214-255): omega first, upsilon second.  Returns pose[7]."""
    u = np.asarray(u, np.float64)
    th = math.sqrt(float(u[:3] @ u[:3]))
    O = PB.skew(u[:3])
    O2 = O @ O
    if th < 0.00001:
        R = np.eye(3) + O + O2
        V = R
    else:
        R = np.eye(3) + math.sin(th) / th * O + (1 - math.cos(th)) / (th * th) * O2
        V = np.eye(3) + (1 - math.cos(th)) / (th * th) * O + (th - math.sin(th)) / (th ** 3) * O2
    q, _ = PB.quat_from_matrix(R)
    return np.concatenate([q, V @ u[3:6]])


def camera_centre(T):
    """KeyFrame::SetPose's Ow = -Rwc * tcw on the float 4 x 4 (src/KeyFrame.cc:71-72): one gemm with alpha -1."""
    T = np.asarray(T, np.float32).reshape(4, 4)
    return CV.mat(T[:3, :3].T, T[:3, 3:4], alpha=-1.0)[:, 0]


# ---------------------------------------------------------------- edges

def project(cam, P, stereo):
    """cam_project of both edge classes on P[..., 3] (camera frame).  The stereo edge carries `const float invz`."""
    fx, fy, cx, cy, bf = cam
    z = P[..., 2]
    with np.errstate(all="ignore"):
        invz = np.where(stereo, (1.0 / z).astype(np.float32).astype(np.float64), 1.0 / z)
        u = np.where(stereo, P[..., 0] * invz * fx + cx, P[..., 0] / z * fx + cx)
        v = np.where(stereo, P[..., 1] * invz * fy + cy, P[..., 1] / z * fy + cy)
        return np.stack([u, v, u - bf * invz], -1)


def edge_errors(cam, R, t, X, obs, stereo):
    """error[..., 3] (third entry 0 on a mono edge) and the camera-frame point."""
    P = np.einsum("eij,ej->ei", R, X) + t
    e = obs - project(cam, P, stereo)
    e[..., 2] = np.where(stereo, e[..., 2], 0.0)
    return e, P


def jacobians(cam, R, P, stereo):
    """(Ji[e, 3, 3] w.r.t. the point, Jj[e, 3, 6] w.r.t. the pose) of linearizeOplus (types_six_dof_expmap.cpp:103-139, :188-234);
    row 2 is zero on a mono edge."""
    fx, fy, cx, cy, bf = cam
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    z2 = z * z
    n = len(x)
    Jj = np.zeros((n, 3, 6))
    Jj[:, 0, 0] = x * y / z2 * fx
    Jj[:, 0, 1] = -(1 + x * x / z2) * fx
    Jj[:, 0, 2] = y / z * fx
    Jj[:, 0, 3] = -1.0 / z * fx
    Jj[:, 0, 5] = x / z2 * fx
    Jj[:, 1, 0] = (1 + y * y / z2) * fy
    Jj[:, 1, 1] = -x * y / z2 * fy
    Jj[:, 1, 2] = -x / z * fy
    Jj[:, 1, 4] = -1.0 / z * fy
    Jj[:, 1, 5] = y / z2 * fy
    Jj[:, 2, 0] = Jj[:, 0, 0] - bf * y / z2
    Jj[:, 2, 1] = Jj[:, 0, 1] + bf * x / z2
    Jj[:, 2, 2] = Jj[:, 0, 2]
    Jj[:, 2, 3] = Jj[:, 0, 3]
    Jj[:, 2, 5] = Jj[:, 0, 5] - bf / z2
    Ji = np.zeros((n, 3, 3))
    for c in range(3):
        Ji[:, 0, c] = -fx * R[:, 0, c] / z + fx * x * R[:, 2, c] / z2
        Ji[:, 1, c] = -fy * R[:, 1, c] / z + fy * y * R[:, 2, c] / z2
        Ji[:, 2, c] = Ji[:, 0, c] - bf * R[:, 2, c] / z2
    Jj[:, 2, :] *= stereo[:, None]
    Ji[:, 2, :] *= stereo[:, None]
    return Ji, Jj


def huber(chi, delta):
    """RobustKernelHuber::robustify (core/robust_kernel_impl.cpp:78-91): (rho, rho')."""
    dsqr = delta * delta
    with np.errstate(all="ignore"):
        sq = np.sqrt(chi)
        big = chi > dsqr
        return np.where(big, 2 * sq * delta - dsqr, chi), np.where(big, delta / sq, 1.0)


def inverse3(D):
    """Eigen's 3 x 3 inverse(): cofactors over the determinant."""
    c = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            c[i, j] = D[i1, j1] * D[i2, j2] - D[i1, j2] * D[i2, j1]
    det = D[0, 0] * c[0, 0] + D[0, 1] * c[0, 1] + D[0, 2] * c[0, 2]
    with np.errstate(all="ignore"):
        return c.T * (1.0 / det)


def ldlt_solve(S, b):
    """Dense LDLT without pivoting; fails (None) only on an exactly zero pivot, as SimplicialLDLT does (a NaN pivot goes on)."""
    n = len(b)
    L = np.array(S, np.float64)
    d = np.zeros(n)
    with np.errstate(all="ignore"):
        for k in range(n):
            d[k] = L[k, k]
            if d[k] == 0.0:
                return None
            L[k + 1:, k] = L[k + 1:, k] / d[k]
            for j in range(k + 1, n):
                L[j:, j] -= L[j:, k] * (d[k] * L[j, k])
        y = np.array(b, np.float64)
        for k in range(n):
            y[k + 1:] -= L[k + 1:, k] * y[k]
        y = y / d
        for k in range(n - 1, -1, -1):
            y[k] -= L[k + 1:, k] @ y[k + 1:]
    return y


# ---------------------------------------------------------------- the problem

class Problem:
    """Vertices, edges and levels of one call.  Built by build(); the solver below works on it."""


def build(kfs, role, Tcw, row, n_rows, obs_off, obs_kf, obs_idx, pos, inv_sigma2, nlevels):
    """Edges from the lists, with the checks only the device can make.  kfs: list of (keys_un record array, u_right float32[n])."""
    p = Problem()
    n_kfs, n_pts, n_obs = len(kfs), len(obs_off) - 1, len(obs_kf)
    role = np.asarray(role, np.uint8)
    p.role, p.n_kfs, p.n_pts, p.n_obs = role, n_kfs, n_pts, n_obs
    p.status = 0
    p.code = np.zeros(n_obs, np.uint8)
    p.e_pt = np.full(n_obs, -1, np.int64)
    p.e_kf = np.zeros(n_obs, np.int64)
    p.obs = np.zeros((n_obs, 3))
    p.stereo = np.zeros(n_obs, bool)
    p.info = np.zeros(n_obs)
    p.valid = np.zeros(n_obs, bool)
    p.row = np.arange(n_pts) if row is None else np.asarray(row, np.int64)
    p.pt_ok = np.zeros(n_pts, bool)
    if (role > FIXED).any():
        p.status = ERR_INVALID
    for q in range(n_pts):
        a, b = int(obs_off[q]), int(obs_off[q + 1])
        if a < 0 or b < a or b > n_obs:
            p.status = ERR_INVALID
            continue
        if not 0 <= p.row[q] < n_rows:
            p.status = ERR_INVALID
            p.code[a:b] = CODE_FAULTY
            continue
        p.pt_ok[q] = True
        for j in range(a, b):
            k, i = int(obs_kf[j]), int(obs_idx[j])
            if not 0 <= k < n_kfs or role[k] > FIXED:
                p.code[j] = CODE_FAULTY
                continue
            if role[k] == SKIP:
                p.code[j] = CODE_SKIPPED
                continue
            keys, ur = kfs[k]
            if not 0 <= i < len(keys) or not 0 <= int(keys["octave"][i]) < nlevels:
                p.code[j] = CODE_FAULTY
                continue
            p.e_pt[j], p.e_kf[j] = q, k
            p.stereo[j] = not (ur[i] < 0)
            p.obs[j] = (float(keys["x"][i]), float(keys["y"][i]), float(ur[i]) if p.stereo[j] else 0.0)
            p.info[j] = float(inv_sigma2[int(keys["octave"][i])])
            p.valid[j] = True
    if (p.code == CODE_FAULTY).any():
        p.status = ERR_INVALID
    p.level = np.zeros(n_obs, np.int64)
    p.pose = np.zeros((n_kfs, 7))
    for k in range(n_kfs):
        if SKIP < role[k] <= FIXED:
            p.pose[k] = PB.pose_from_cv(Tcw[k])[0]
    p.X = np.zeros((n_pts, 3))
    ok = np.nonzero(p.pt_ok)[0]
    p.X[ok] = np.asarray(pos, np.float32)[p.row[ok]].astype(np.float64)
    p.reduced = []                    # size of the reduced system per optimize()
    p.last_rejected = []              # per optimize(): its last trial was not accepted, so chi2() and the estimates are of two states
    p.chi2 = np.zeros(n_obs)          # BaseEdge::chi2() at the last computeActiveErrors that saw the edge
    return p


def _rot(pose):
    return np.stack([PB.quat_to_matrix(q) for q in pose]) if len(pose) else np.zeros((0, 3, 3))


def errors(p, cam, pose, X, act):
    R = _rot(pose)
    e, P = edge_errors(cam, R[p.e_kf[act]], pose[p.e_kf[act], 4:7], X[p.e_pt[act]], p.obs[act], p.stereo[act])
    chi = p.info[act] * (e * e).sum(-1)
    return e, P, chi, R


def robust_total(p, act, chi, robust):
    if not robust:
        return float(np.cumsum(chi)[-1]) if len(chi) else 0.0
    rho = np.where(p.stereo[act], huber(chi, DELTA_STEREO)[0], huber(chi, DELTA_MONO)[0])
    return float(np.cumsum(rho)[-1]) if len(rho) else 0.0


class System:
    pass


def linearize(p, cam, pose, X, act, robust, all_free=False):
    """buildSystem: Hpp / b_p per active free keyframe, Hll / b_l per active point, Hpl per edge on a free keyframe."""
    s = System()
    e, P, chi, R = errors(p, cam, pose, X, act)
    Ji, Jj = jacobians(cam, R[p.e_kf[act]], P, p.stereo[act])
    w = np.ones(len(act))
    if robust:
        w = np.where(p.stereo[act], huber(chi, DELTA_STEREO)[1], huber(chi, DELTA_MONO)[1])
    wi = w * p.info[act]
    s.act = act
    s.free = np.nonzero(p.role == LOCAL)[0]
    if not all_free:
        s.free = np.array([k for k in s.free if (p.e_kf[act] == k).any()], np.int64)   # a vertex without an active edge is not active
    s.red = {int(k): r for r, k in enumerate(s.free)}
    s.pts = np.unique(p.e_pt[act])
    s.Hll = np.zeros((p.n_pts, 3, 3))
    s.bl = np.zeros((p.n_pts, 3))
    s.Hpp = np.zeros((p.n_kfs, 6, 6))
    s.bp = np.zeros((p.n_kfs, 6))
    np.add.at(s.Hll, p.e_pt[act], np.einsum("eki,e,ekj->eij", Ji, wi, Ji))
    np.add.at(s.bl, p.e_pt[act], -np.einsum("eki,e,ek->ei", Ji, wi, e))
    np.add.at(s.Hpp, p.e_kf[act], np.einsum("eki,e,ekj->eij", Jj, wi, Jj))
    np.add.at(s.bp, p.e_kf[act], -np.einsum("eki,e,ek->ei", Jj, wi, e))
    s.Hpl = np.einsum("eki,e,ekj->eij", Jj, wi, Ji)     # [e, 6, 3]
    s.on_free = np.array([int(k) in s.red for k in p.e_kf[act]], bool)
    return s


def lambda_init(p, s):
    m = 0.0
    for k in s.free:
        for d in np.abs(np.diag(s.Hpp[k])):
            m = max(m, d) if d == d else m
    for q in s.pts:
        for d in np.abs(np.diag(s.Hll[q])):
            m = max(m, d) if d == d else m
    return 1e-5 * m


def reduce_system(p, s, lam):
    """The Schur part of BlockSolver::solve: (S, bschur, Dinv per point, lists of (edge position, reduced index) per point)."""
    n = 6 * len(s.free)
    S = np.zeros((n, n))
    for r, k in enumerate(s.free):
        S[6 * r:6 * r + 6, 6 * r:6 * r + 6] = s.Hpp[k] + lam * np.eye(6)
    coeff = np.zeros(n)
    Dinv = {}
    lists = {}
    for a in np.nonzero(s.on_free)[0]:
        lists.setdefault(int(p.e_pt[s.act[a]]), []).append((int(a), s.red[int(p.e_kf[s.act[a]])]))
    for q in s.pts:
        q = int(q)
        Dinv[q] = inverse3(s.Hll[q] + lam * np.eye(3))
        db = Dinv[q] @ s.bl[q]
        col = lists.get(q, [])
        for a, r1 in col:
            BDinv = s.Hpl[a] @ Dinv[q]
            coeff[6 * r1:6 * r1 + 6] += s.Hpl[a] @ db
            for b, r2 in col:
                if r2 >= r1:
                    blk = BDinv @ s.Hpl[b].T
                    S[6 * r1:6 * r1 + 6, 6 * r2:6 * r2 + 6] -= blk
                    if r2 > r1:
                        S[6 * r2:6 * r2 + 6, 6 * r1:6 * r1 + 6] -= blk.T
    bs = np.concatenate([s.bp[k] for k in s.free]) - coeff if n else np.zeros(0)
    return S, bs, Dinv, lists


def solve(p, s, lam):
    """(xp[len(free), 6], xl[n_pts, 3]) or None when the reduced system meets a zero pivot."""
    S, bs, Dinv, lists = reduce_system(p, s, lam)
    xp = ldlt_solve(S, bs)
    if xp is None:
        return None
    xp = xp.reshape(-1, 6)
    xl = np.zeros((p.n_pts, 3))
    for q in s.pts:
        q = int(q)
        cl = s.bl[q].copy()
        for a, r in lists.get(q, []):
            cl -= s.Hpl[a].T @ xp[r]
        xl[q] = Dinv[q] @ cl
    return xp, xl


def optimize(p, cam, iterations, robust, quirks=ALL_QUIRKS, log=None):
    """SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg (core/optimization_algorithm_levenberg.cpp:59-193)
    over the level-0 edges.  Returns (iterations run, trials, chi2 at entry, chi2 at exit, lambda)."""
    act = np.nonzero(p.valid & (p.level == 0))[0]
    if len(act) == 0:
        return 0, 0, 0.0, 0.0, None
    all_free = "orphans" not in quirks   # the "fix": a keyframe without a level-0 edge takes part with a zero block (plus lambda)
    _, _, chi, _ = errors(p, cam, p.pose, p.X, act)
    chi_at_est = chi
    p.chi2[act] = chi
    current = robust_total(p, act, chi, robust)
    start = current
    s = linearize(p, cam, p.pose, p.X, act, robust, all_free)
    p.reduced.append(6 * len(s.free))
    lam, ni, bad = -1.0, 2.0, 0
    xp, xl = np.zeros((len(s.free), 6)), np.zeros((p.n_pts, 3))
    runs = trials = 0
    accepted = True
    for it in range(iterations):
        runs += 1
        p.chi2[act] = chi_at_est                                     # computeActiveErrors at the current estimate
        ini = current
        if it == 0:
            lam, ni, bad = lambda_init(p, s), 2.0, 0
        rho, qmax = 0.0, 0
        while True:
            sol = solve(p, s, lam)
            if sol is not None:
                xp, xl = sol                                          # a failed solve leaves x as it was
            scale = 0.0
            for r, k in enumerate(s.free):
                for j in range(6):
                    scale += xp[r, j] * (lam * xp[r, j] + s.bp[k, j])
            for q in s.pts:
                for j in range(3):
                    scale += xl[q, j] * (lam * xl[q, j] + s.bl[q, j])
            scale += 1e-3
            pose_t, X_t = p.pose.copy(), p.X.copy()
            for r, k in enumerate(s.free):
                pose_t[k] = PB.se3_mul(se3_exp(xp[r]), p.pose[k])
            X_t[s.pts] = p.X[s.pts] + xl[s.pts]
            _, _, chi_t, _ = errors(p, cam, pose_t, X_t, act)
            p.chi2[act] = chi_t
            temp = robust_total(p, act, chi_t, robust) if sol is not None else DBL_MAX
            with np.errstate(all="ignore"):
                rho = (current - temp) / scale
            if rho > 0 and np.isfinite(temp):
                r21 = 2 * rho - 1
                lam *= max(1.0 / 3.0, min(1.0 - r21 * r21 * r21, 2.0 / 3.0))
                ni = 2.0
                current = temp
                accepted = True
                p.pose, p.X, chi_at_est = pose_t, X_t, chi_t
                s = linearize(p, cam, p.pose, p.X, act, robust, all_free)
            else:
                lam *= ni
                ni *= 2
                accepted = False
            qmax += 1
            if log is not None:
                log.append((it, qmax, rho, temp, lam))
            if not (rho < 0 and qmax < 10):
                break
        trials += qmax
        if qmax == 10 or rho == 0:
            break
        bad = bad + 1 if (ini - current) * 1e3 < ini else 0
        if bad >= 3:
            break
    p.last_rejected.append(not accepted)
    return runs, trials, start, current, lam


def classify(p, cam, quirks):
    """chi2() > 5.991 / 7.815 || !isDepthPositive() over every edge: chi2 as the last evaluation left it, depth at the current estimates."""
    ed = np.nonzero(p.valid)[0]
    _, P, chi_now, _ = errors(p, cam, p.pose, p.X, ed)
    if "stale_chi2" not in quirks:     # the "fix": every edge's chi2 recomputed at the current estimates
        p.chi2[ed] = chi_now
    chi = p.chi2[ed]
    out = np.zeros(p.n_obs, bool)
    out[ed] = (chi > np.where(p.stereo[ed], CHI2_STEREO, CHI2_MONO)) | ~(P[:, 2] > 0.0)
    margin = dict(chi=np.abs(chi / np.where(p.stereo[ed], CHI2_STEREO, CHI2_MONO) - 1.0).min() if len(ed) else np.inf,
                  depth=np.abs(P[:, 2]).min() if len(ed) else np.inf)
    return out, margin


def local_bundle_adjustment(kfs, role, Tcw, row, n_rows, obs_off, obs_kf, obs_idx, pos, cam, inv_sigma2, nlevels=8, max_free_kfs=None,
                            quirks=ALL_QUIRKS, iterations=(5, 10)):
    """Everything the call returns, plus the per-round counts and the classification margins.  cam = (fx, fy, cx, cy, bf)."""
    Tcw = np.array(Tcw, np.float32).reshape(-1, 16)
    pos = np.array(pos, np.float32).reshape(-1, 3)
    role = np.asarray(role, np.uint8)
    n_obs = len(obs_kf)
    out = dict(Tcw=Tcw.copy(), pos=pos.copy(), Ow=np.full((len(role), 3), np.nan, np.float32), rewritten=np.zeros(len(role), bool),
               edge_code=None, edge_chi2=None, erase=np.zeros((0, 2), np.int32), info=None, status=0, iterations=[0, 0], trials=[0, 0],
               margins=[])
    if max_free_kfs is not None and int((role == LOCAL).sum()) > max_free_kfs:
        out["status"] = ERR_CAPACITY
        return out
    p = build(kfs, role, Tcw, row, n_rows, obs_off, obs_kf, obs_idx, pos, inv_sigma2, nlevels)
    out["status"] = p.status
    out["edge_code"] = p.code
    n_mono, n_stereo = int((p.valid & ~p.stereo).sum()), int((p.valid & p.stereo).sum())
    info = dict(n_mono=n_mono, n_stereo=n_stereo, n_free=0, n_points=0, iterations=[0, 0], trials=[0, 0], chi2_start=0.0, chi2_first=0.0,
                chi2_second=0.0, lambda_last=0.0)
    out["info"] = info
    out["edge_chi2"] = np.zeros(n_obs)
    if not p.valid.any():
        return out
    info["n_free"] = int(len(set(p.e_kf[p.valid].tolist()) & set(np.nonzero(role == LOCAL)[0].tolist())))
    info["n_points"] = int(len(np.unique(p.e_pt[p.valid])))
    r1 = optimize(p, cam, iterations[0], True, quirks)
    flagged, m1 = classify(p, cam, quirks)
    p.level[flagged] = 1
    p.code[flagged] |= CODE_LEVEL1
    r2 = optimize(p, cam, iterations[1], False, quirks)
    erase, m2 = classify(p, cam, quirks)
    p.code[erase] |= CODE_ERASE
    info["iterations"], info["trials"] = [r1[0], r2[0]], [r1[1], r2[1]]
    info["chi2_start"], info["chi2_first"], info["chi2_second"] = r1[2], r1[3], r2[3]
    info["lambda_last"] = r2[4] if r2[4] is not None else r1[4]
    out["iterations"], out["trials"], out["margins"] = info["iterations"], info["trials"], [m1, m2]
    out["edge_chi2"] = p.chi2.copy()
    order = [j for j in np.nonzero(erase)[0] if not p.stereo[j]] + [j for j in np.nonzero(erase)[0] if p.stereo[j]]
    out["erase"] = np.array([(p.e_kf[j], p.e_pt[j]) for j in order], np.int32).reshape(-1, 2)
    for k in range(len(role)):
        rewrite = role[k] in (LOCAL, LOCAL_HELD) or ("fixed_bits" not in quirks and role[k] == FIXED)
        if role[k] == LOCAL_HELD and "held_rewrite" not in quirks:
            rewrite = False
        if rewrite:
            out["Tcw"][k] = PB.pose_to_cv(p.pose[k]).reshape(16)
            out["Ow"][k] = camera_centre(out["Tcw"][k])
            out["rewritten"][k] = True
    ok = np.nonzero(p.pt_ok)[0]
    out["pos"][p.row[ok]] = p.X[ok].astype(np.float32)
    out["poses"], out["X"], out["reduced"] = p.pose, p.X, p.reduced
    out["last_rejected"] = p.last_rejected
    return out
