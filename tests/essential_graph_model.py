"""Float64 model of orbfe_enqueue_optimize_essential_graph (include/orbfe.h): Optimizer::OptimizeEssentialGraph (reference
src/Optimizer.cc:825-1088) on flattened fields, with g2o's Sim3 algebra and Sim3::log (Thirdparty/g2o/g2o/types/sim3.h:148-230),
EdgeSim3::computeError (types_seven_dof_expmap.h:106-114), BaseBinaryEdge's NUMERIC Jacobians (central differences, delta 1e-9, through
oplus), constructQuadraticForm without a robust kernel and with information = identity, and OptimizationAlgorithmLevenberg with the user's
initial lambda.  It is the reference of tests/test_essential_graph_model.py (which proves it), tests/test_essential_graph_plan.py,
tests/test_essential_blocks.py and tests/test_essential_graph_device.py.

Edge-sequential: H, b and chi2 are Python loops over the edges in input order; the linear system is DENSE and solved by
numpy.linalg.solve (the device follows a block-sparse plan: the elimination order changes rounding only).  Scalars are Python floats:
no fused multiply-add, so the stages without a libm call (recovery, point correction) give the device's bits.  The Sim3 algebra and
the exponential are tests/sim3_opt_model.py's.  A Sim3 is (q, t, s), q = (x, y, z, w), never normalised.
"""
import math

import numpy as np

from tests import sim3_opt_model as S3

ERR_INVALID = -1
EDGE_INDEX, EDGE_SIM3 = 1, 2
LAMBDA_INIT = float(np.float32(1.0e-16))
DBL_MAX = np.finfo(np.float64).max
PLAN_MAGIC = 0x31504745
HEADER_WORDS = 20
HEADER_FIELDS = ("magic", "n_kfs", "fixed_kf", "n_edges", "n_free", "n_lblocks", "n_slot_edges", "n_updates", "blob_bytes", "off_order", "off_pos",
                 "off_colptr", "off_rowidx", "off_edge_slots", "off_slot_ptr", "off_slot_edges", "off_upd_ptr", "off_upd")


# ---------------------------------------------------------------- Sim3::log
def to_rotation(q):
    """Eigen's Quaternion::toRotationMatrix, operation by operation."""
    x, y, z, w = (float(v) for v in q)
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]]


def lu3_solve(W, t):
    """PartialPivLU<Matrix3d>::solve as DESIGN.md section 4s states it: the first largest |entry| of the column is the pivot."""
    W = [[float(v) for v in r] for r in W]
    c = [float(v) for v in t]
    for k in range(3):
        piv, best = k, abs(W[k][k])
        for i in range(k + 1, 3):
            if abs(W[i][k]) > best:
                best, piv = abs(W[i][k]), i
        if piv != k:
            W[k], W[piv] = W[piv], W[k]
            c[k], c[piv] = c[piv], c[k]
        if best != 0.0:
            for i in range(k + 1, 3):
                W[i][k] /= W[k][k]
        for i in range(k + 1, 3):
            for j in range(k + 1, 3):
                W[i][j] -= W[i][k] * W[k][j]
    c[1] -= W[1][0] * c[0]
    c[2] -= W[2][0] * c[0] + W[2][1] * c[1]
    x2 = c[2] / W[2][2]
    x1 = (c[1] - W[1][2] * x2) / W[1][1]
    x0 = (c[0] - (W[0][1] * x1 + W[0][2] * x2)) / W[0][0]
    return [x0, x1, x2]


def log_branch(S):
    """(|sigma| < 1e-5, d > 1 - 1e-5) of Sim3::log."""
    R = to_rotation(S[0])
    return (abs(math.log(S[2])) < 0.00001, 0.5 * (R[0][0] + R[1][1] + R[2][2] - 1) > 1 - 0.00001)


def sim3_log(S):
    """Sim3::log(), all four branches as written."""
    q, t, s = S
    sigma = math.log(s)
    R = to_rotation(q)
    d = 0.5 * (R[0][0] + R[1][1] + R[2][2] - 1)
    dR = [R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]]
    eps = 0.00001
    small = d > 1 - eps
    theta = 0.0
    if small:
        k = 0.5
    else:
        theta = math.acos(d)
        k = theta / (2 * math.sqrt(1 - d * d))
    om = [k * dR[0], k * dR[1], k * dR[2]]
    if abs(sigma) < eps:
        C = 1.0
        if small:
            A, B = 1. / 2., 1. / 6.
        else:
            theta2 = theta * theta
            A = (1 - math.cos(theta)) / theta2
            B = (theta - math.sin(theta)) / (theta2 * theta)
    else:
        C = (s - 1) / sigma
        if small:
            sigma2 = sigma * sigma
            A = ((sigma - 1) * s + 1) / sigma2
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
        else:
            theta2 = theta * theta
            a, b = s * math.sin(theta), s * math.cos(theta)
            c = theta2 + sigma * sigma
            A = (a * sigma + (1 - b) * theta) / (theta * c)
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2
    O = [[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]]
    W = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            o2 = ((B * O[i][0]) * O[0][j] + (B * O[i][1]) * O[1][j]) + (B * O[i][2]) * O[2][j]
            W[i][j] = (A * O[i][j] + o2) + C * (1.0 if i == j else 0.0)
    ups = lu3_solve(W, t)
    return [om[0], om[1], om[2], ups[0], ups[1], ups[2], sigma]


def finite(S):
    return all(math.isfinite(v) for v in list(S[0]) + list(S[1]) + [S[2]])


def sim3_from_Tcw(T):
    """Sim3(Converter::toMatrix3d(Rcw), Converter::toVector3d(tcw), 1.0) of a float row."""
    T = np.asarray(T, np.float32).reshape(4, 4)
    return S3.sim3(T[:3, :3].astype(np.float64), T[:3, 3].astype(np.float64), 1.0)


# ---------------------------------------------------------------- the edge
def edge_error(C, Si, Sj_inv):
    """EdgeSim3::computeError: log(C * S_i * S_j.inverse())."""
    return sim3_log(S3.sim3_mul(S3.sim3_mul(C, Si), Sj_inv))


def perturbed(est, fix_scale):
    """The 14 oplus results of linearizeOplus for one vertex, [2 d + (0: +, 1: -)], each with its inverse, then the estimate."""
    out = []
    for d in range(7):
        for sign in (1.0, -1.0):
            u = [0.0] * 7
            u[d] = sign * 1e-9
            S = S3.oplus(u, fix_scale, est)
            out.append((S, S3.sim3_inverse(S)))
    out.append((est, S3.sim3_inverse(est)))
    return out


def edge_linearize(C, pert_i, pert_j, free_i, free_j):
    """e (7), Ji, Jj (7 x 7, row = error component); a fixed end's block is zero."""
    Si, Sj_inv = pert_i[14][0], pert_j[14][1]
    e = np.array(edge_error(C, Si, Sj_inv))
    scalar = 1.0 / (2 * 1e-9)
    Ji, Jj = np.zeros((7, 7)), np.zeros((7, 7))
    for d in range(7):
        if free_i:
            ep, em = edge_error(C, pert_i[2 * d][0], Sj_inv), edge_error(C, pert_i[2 * d + 1][0], Sj_inv)
            Ji[:, d] = [scalar * (p - m) for p, m in zip(ep, em)]
        if free_j:
            ep, em = edge_error(C, Si, pert_j[2 * d][1]), edge_error(C, Si, pert_j[2 * d + 1][1])
            Jj[:, d] = [scalar * (p - m) for p, m in zip(ep, em)]
    return e, Ji, Jj


# ---------------------------------------------------------------- the problem
class Problem:
    """Vertices, edge codes and measurements as the kernel forms them before the first iteration."""

    def __init__(self, Tcw, fixed_kf, edge_i, edge_j, edge_kind, corrected=None, has_corrected=None, noncorrected=None, has_noncorrected=None):
        Tcw = np.asarray(Tcw, np.float32).reshape(-1, 16)
        n = self.n_kfs = len(Tcw)
        self.fixed = int(fixed_kf)
        self.init, self.vbad = [], []
        for v in range(n):
            S = S3.unpack(corrected[v]) if has_corrected is not None and has_corrected[v] else sim3_from_Tcw(Tcw[v])
            self.init.append(S)
            self.vbad.append(not finite(S))
        self.edges, self.code, self.meas = [], [], []
        for i, j, kind in zip(edge_i, edge_j, edge_kind):
            i, j = int(i), int(j)
            code, C = 0, None
            if i < 0 or i >= n or j < 0 or j >= n or i == j:
                code = EDGE_INDEX
            else:
                nc = kind != 0 and has_noncorrected is not None
                Si = S3.unpack(noncorrected[i]) if nc and has_noncorrected[i] else self.init[i]
                Sj = S3.unpack(noncorrected[j]) if nc and has_noncorrected[j] else self.init[j]
                if self.vbad[i] or self.vbad[j] or not finite(Si) or not finite(Sj):
                    code = EDGE_SIM3
                else:
                    C = S3.sim3_mul(Sj, S3.sim3_inverse(Si))
            self.edges.append((i, j))
            self.code.append(code)
            self.meas.append(C)
        self.free = [v for v in range(n) if v != self.fixed]
        self.col = {v: k for k, v in enumerate(self.free)}   # the model's own (identity) order
        self.invalid = any(self.code) or any(self.vbad)

    def active(self):
        return [e for e in range(len(self.edges)) if not self.code[e]]

    def chi2(self, est):
        chi = 0.0
        for e in self.active():
            i, j = self.edges[e]
            err = edge_error(self.meas[e], est[i], S3.sim3_inverse(est[j]))
            chi += sum(v * v for v in err)
        return chi

    def linearize(self, est, fix_scale):
        """Dense H (7 n_free square), b, chi2 and the per-edge (e, Ji, Jj), in edge order."""
        nf = len(self.free)
        H, b, chi = np.zeros((7 * nf, 7 * nf)), np.zeros(7 * nf), 0.0
        pert = {v: perturbed(est[v], fix_scale) for v in range(self.n_kfs) if not self.vbad[v]}
        blocks = {}
        for e in self.active():
            i, j = self.edges[e]
            err, Ji, Jj = edge_linearize(self.meas[e], pert[i], pert[j], i != self.fixed, j != self.fixed)
            blocks[e] = (err, Ji, Jj)
            chi += float(err @ err)
            if i != self.fixed:
                a = 7 * self.col[i]
                H[a:a + 7, a:a + 7] += Ji.T @ Ji
                b[a:a + 7] -= Ji.T @ err
            if j != self.fixed:
                c = 7 * self.col[j]
                H[c:c + 7, c:c + 7] += Jj.T @ Jj
                b[c:c + 7] -= Jj.T @ err
            if i != self.fixed and j != self.fixed:
                H[a:a + 7, c:c + 7] += Ji.T @ Jj
                H[c:c + 7, a:a + 7] += Jj.T @ Ji
        return H, b, chi, blocks

    def apply(self, est, x, fix_scale):
        out = list(est)
        for v in self.free:
            if not self.vbad[v]:
                out[v] = S3.oplus(x[7 * self.col[v]: 7 * self.col[v] + 7], fix_scale, est[v])
        return out


def optimize(P, iterations, fix_scale, lambda_init=LAMBDA_INIT, trace=None):
    """SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg (section 4a's loop, lambda from the user's value).
    Returns (final estimates, info dict).  trace, a list, receives (iteration, trial, rho, temp_chi, lambda) per trial."""
    est = list(P.init)
    info = dict(iterations=0, trials=0, n_active_edges=len(P.active()), chi2_start=0.0, chi2_end=0.0, lambda_last=lambda_init)
    if not P.active() or not P.free:
        return est, info
    lam, ni, lm_bad = lambda_init, 2.0, 0
    x = np.zeros(7 * len(P.free))
    current = 0.0
    for it in range(iterations):
        info["iterations"] += 1
        H, b, chi, _ = P.linearize(est, fix_scale)
        if it == 0:
            info["chi2_start"] = chi
            lam, ni, lm_bad = lambda_init, 2.0, 0
        current = chi
        ini = current
        rho, qmax = 0.0, 0
        while True:
            try:
                xs = np.linalg.solve(H + lam * np.eye(len(b)), b)
                ok = bool(np.all(np.isfinite(xs)))
            except np.linalg.LinAlgError:
                ok = False
            if ok:
                x = xs
            scale = float(np.sum(x * (lam * x + b))) + 1e-3
            temp = DBL_MAX
            if ok:
                trial = P.apply(est, x, fix_scale)
                temp = P.chi2(trial)
            info["trials"] += 1
            rho = (current - temp) / scale
            if trace is not None:
                trace.append((it, qmax, rho, temp, lam))
            if rho > 0 and math.isfinite(temp):
                r21 = 2 * rho - 1
                alpha = min(1.0 - r21 * r21 * r21, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni = 2.0
                current = temp
                if ok:
                    est = trial
            else:
                lam *= ni
                ni *= 2
            qmax += 1
            if not (rho < 0 and qmax < 10):
                break
        if qmax == 10 or rho == 0:
            break
        lm_bad = lm_bad + 1 if (ini - current) * 1e3 < ini else 0
        if lm_bad >= 3:
            break
    info["chi2_end"], info["lambda_last"] = current, lam
    return est, info


# ---------------------------------------------------------------- recovery and points (no libm: the device's bits)
def recover_pose(S):
    """(Tcw float32[16], Ow float32[3]): toRotationMatrix(), t * (1. / s), Converter::toCvSE3; Ow = -R^T t as the kernel patches it."""
    R = to_rotation(S[0])
    inv = 1.0 / S[2]
    T = np.zeros(16, np.float32)
    for i in range(3):
        for j in range(3):
            T[4 * i + j] = np.float32(R[i][j])
        T[4 * i + 3] = np.float32(S[1][i] * inv)
    T[15] = 1.0
    Ow = np.zeros(3, np.float32)
    for i in range(3):
        s = 0.0
        for m in range(3):
            s += float(T[4 * m + i]) * float(T[4 * m + 3])
        Ow[i] = np.float32(-1.0 * s)
    return T, Ow


def correct_point(Srw, correctedSwr, p):
    m = S3.sim3_map(Srw, float(p[0]), float(p[1]), float(p[2]))
    o = S3.sim3_map(correctedSwr, *m)
    return np.array(o, np.float64).astype(np.float32)


def finish(P, final, Tcw, pos, pt_ref, pt_valid):
    """Recovery and point correction from `final` estimates (the model's own, or the device's): Tcw, Ow, pos, pt_code, status bit."""
    T = np.asarray(Tcw, np.float32).reshape(-1, 16).copy()
    Ow = np.zeros((P.n_kfs, 3), np.float32)
    inv = [None] * P.n_kfs
    for v in range(P.n_kfs):
        if P.vbad[v]:
            continue
        T[v], Ow[v] = recover_pose(final[v])
        inv[v] = S3.sim3_inverse(final[v])
    pos = np.asarray(pos, np.float32).reshape(-1, 3).copy()
    code = np.zeros(len(pos), np.uint8)
    for q in range(len(pos)):
        if not pt_valid[q]:
            continue
        r = int(pt_ref[q])
        if r < 0 or r >= P.n_kfs:
            code[q] = 1
        elif not P.vbad[r]:
            pos[q] = correct_point(P.init[r], inv[r], pos[q])
    return T, Ow, pos, code


def run(Tcw, fixed_kf, edge_i, edge_j, edge_kind, corrected=None, has_corrected=None, noncorrected=None, has_noncorrected=None, iterations=20,
        fix_scale=False, lambda_init=LAMBDA_INIT, pos=None, pt_ref=None, pt_valid=None):
    """The whole call; the dict of Context.optimize_essential_graph."""
    P = Problem(Tcw, fixed_kf, edge_i, edge_j, edge_kind, corrected, has_corrected, noncorrected, has_noncorrected)
    final, info = optimize(P, iterations, fix_scale, lambda_init)
    pos = np.zeros((0, 3), np.float32) if pos is None else pos
    T, Ow, po, pcode = finish(P, final, Tcw, pos, pt_ref, pt_valid)
    return dict(Tcw=T, Ow=Ow, pos=po, sim3=np.array([S3.pack(S) for S in final]).reshape(-1, 8), edge_code=np.array(P.code, np.uint8), pt_code=pcode,
                info=info, status=ERR_INVALID if (P.invalid or pcode.any()) else 0, problem=P)


# ---------------------------------------------------------------- the plan, read and followed in numpy
def parse_plan(blob):
    """The planner's blob (int32 words) as a dict of its header fields and sections."""
    w = np.asarray(blob).view(np.int32).reshape(-1)
    h = {k: int(w[i]) for i, k in enumerate(HEADER_FIELDS)}
    nf, nl, ne = h["n_free"], h["n_lblocks"], h["n_edges"]
    sec = lambda off, n: w[off: off + n].copy()
    h.update(order=sec(h["off_order"], nf), pos=sec(h["off_pos"], h["n_kfs"]), colptr=sec(h["off_colptr"], nf + 1), rowidx=sec(h["off_rowidx"], nl),
             edge_slots=sec(h["off_edge_slots"], 4 * ne).reshape(ne, 4), slot_ptr=sec(h["off_slot_ptr"], nf + nl + 1),
             slot_edges=sec(h["off_slot_edges"], h["n_slot_edges"]), upd_ptr=sec(h["off_upd_ptr"], nf + 1), upd=sec(h["off_upd"], 3 * h["n_updates"]).reshape(-1, 3))
    h["n_slots"] = nf + nl
    return h


def plan_assemble(plan, blocks):
    """The slots of H ([n_slots][7][7]) and b ([n_free][7]) from per-edge (e, Ji, Jj), each slot's edges in the plan's order."""
    nf, ns = plan["n_free"], plan["n_slots"]
    Hs, b = np.zeros((ns, 7, 7)), np.zeros((nf, 7))
    for s in range(ns):
        for w in plan["slot_edges"][plan["slot_ptr"][s]: plan["slot_ptr"][s + 1]]:
            e, side = int(w) >> 1, int(w) & 1
            if e not in blocks:
                continue
            err, Ji, Jj = blocks[e]
            if s < nf:
                J = Jj if side else Ji
                Hs[s] += J.T @ J
                b[s] -= J.T @ err
            else:
                Hs[s] += (Ji.T @ Jj) if side else (Jj.T @ Ji)
    return Hs, b


def plan_dense(plan, Hs):
    """The symmetric dense matrix (elimination order) that the slots stand for."""
    nf = plan["n_free"]
    A = np.zeros((7 * nf, 7 * nf))
    for p in range(nf):
        A[7 * p: 7 * p + 7, 7 * p: 7 * p + 7] = Hs[p]
        for q in range(plan["colptr"][p], plan["colptr"][p + 1]):
            r = plan["rowidx"][q]
            A[7 * r: 7 * r + 7, 7 * p: 7 * p + 7] = Hs[nf + q]
            A[7 * p: 7 * p + 7, 7 * r: 7 * r + 7] = Hs[nf + q].T
    return A


def plan_solve(plan, Hs, b, lam=0.0):
    """The kernel's right-looking block LDLT and both substitutions along the plan, in numpy; x in elimination order ([n_free][7])."""
    nf = plan["n_free"]
    F, y = Hs.copy(), b.copy()
    for p in range(nf):
        F[p] += lam * np.eye(7)
    for p in range(nf):
        A = F[p]
        L, D = np.eye(7), np.zeros(7)
        for j in range(7):
            D[j] = A[j, j] - np.sum(L[j, :j] ** 2 * D[:j])
            for i in range(j + 1, 7):
                L[i, j] = (A[i, j] - np.sum(L[i, :j] * L[j, :j] * D[:j])) / D[j]
        F[p] = np.tril(L, -1) + np.diag(D)
        y[p] = np.linalg.solve(L, y[p])
        cb, ce = plan["colptr"][p], plan["colptr"][p + 1]
        for q in range(cb, ce):
            F[nf + q] = np.linalg.solve(L, F[nf + q].T).T / D   # X = B L^-T D^-1
        for a, c, t in plan["upd"][plan["upd_ptr"][p]: plan["upd_ptr"][p + 1]]:
            F[t] -= (F[a] * D) @ F[c].T
        for q in range(cb, ce):
            y[plan["rowidx"][q]] -= F[nf + q] @ y[p]
    for p in range(nf - 1, -1, -1):
        L, D = np.tril(F[p], -1) + np.eye(7), np.diag(F[p]).copy()
        acc = y[p] / D
        for q in range(plan["colptr"][p], plan["colptr"][p + 1]):
            acc -= F[nf + q].T @ y[plan["rowidx"][q]]
        y[p] = np.linalg.solve(L.T, acc)
    return y
