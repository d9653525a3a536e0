"""The device blocks of PoseOptimization (orbslam2_amd/csrc/orbfe_pose_blocks.hpp), one at a time, against float64 references.

tests/test_pose.py compares the whole kernel with the oracle at 1e-5 on the pose.  Levenberg-Marquardt reaches the same optimum
with a wrong H as long as b and chi2 are right, the scenes there take 3 of the 15 pivot exchanges and one of the four quaternion
branches: a wrong off-diagonal of J^T W J, a wrong slot of the transposing reduction, a wrong sym_swap instance or a wrong
non-trace quaternion branch would leave that suite green.  Here tests/pose_blocks/pose_blocks.hip (test-only, the product's
compiler flags) runs se3_from_cv / se3_to_cv, se3_exp, se3_mul, solve_ldlt6 and both eval_pass instances alone.

The references are tests/pose_blocks_model.py.  The CPU tests below check them against the oracle's hooks on the very cases the
GPU tests use, so a reference is proven before a GPU sees it.
"""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import pose_blocks_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
OP_FROM_CV, OP_EXP, OP_MUL, OP_LDLT, OP_EVAL = 1, 2, 3, 4, 5
IN_STRIDE = {OP_FROM_CV: 16, OP_EXP: 6, OP_MUL: 14, OP_LDLT: 28}
OUT_STRIDE = {OP_FROM_CV: 23, OP_EXP: 7, OP_MUL: 7, OP_LDLT: 7, OP_EVAL: 62}
INV_SIGMA2 = (1.0 / (np.float32(1.2) ** np.arange(8, dtype=np.float32)) ** 2).astype(np.float32)


class _EvalIn(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("hdr", "keys", "u_right", "has_point", "Xw", "outlier", "inv_sigma2")] + [("total", C.c_int32)]


def _lib():
    path = os.path.join(HERE, "pose_blocks", "libpose_blocks.so")
    if not os.path.exists(path):
        raise RuntimeError("tests/pose_blocks/libpose_blocks.so is missing: __graft_entry__.build() compiles it")
    L = C.CDLL(path)
    L.pose_blocks_run.restype = C.c_int
    L.pose_blocks_run.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return L


def _run(op, cases):
    a = np.ascontiguousarray(cases, np.float64).reshape(-1, IN_STRIDE[op])
    out = np.zeros((len(a), OUT_STRIDE[op]))
    assert _lib().pose_blocks_run(op, len(a), a.ctypes.data, out.ctypes.data) == 0
    return out


def _hooks():
    L = O.lib()
    L.orc_test_quat_roundtrip.restype = None; L.orc_test_quat_roundtrip.argtypes = [C.c_void_p] * 3
    L.orc_test_se3_exp.restype = None; L.orc_test_se3_exp.argtypes = [C.c_void_p] * 2
    L.orc_test_ldlt6.restype = C.c_int; L.orc_test_ldlt6.argtypes = [C.c_void_p] * 3
    return L


# ================================================================ cases (shared by the CPU and the GPU tests)

def _T(R, t=(0.0, 0.0, 0.0)):
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = np.asarray(R, np.float64).astype(np.float32)
    T[:3, 3] = t
    return T


def from_cv_cases():
    """(name, float32 4x4, expected branch).  Near-180-degree rotations about each axis take the non-trace branches; the tied
    matrices are exact in float: 180 degrees about (1,1,0), (0,1,1), (1,1,1) and 120 degrees about (1,1,1) (trace exactly 0)."""
    cs = [("trace", _T(M.rot((0.3, -0.2, 0.1)), (0.1, -0.2, 0.3)), "trace"),
          ("i0", _T(M.rot((3.1, 0.05, -0.02)), (0.5, 0.0, -0.25)), 0),
          ("i1", _T(M.rot((0.04, 3.12, 0.03)), (-0.4, 0.3, 0.2)), 1),
          ("i2", _T(M.rot((-0.03, 0.02, 3.13)), (0.0, 0.7, -0.6)), 2),
          ("i0_far", _T(M.rot((2.2, 2.2, 0.1))), None),
          ("generic", _T(M.rot((1.5, -1.7, 2.0)), (3.0, -2.0, 1.0)), None),
          ("tie_m00_m11", _T([[0, 1, 0], [1, 0, 0], [0, 0, -1]]), 0),
          ("tie_m11_m22", _T([[-1, 0, 0], [0, 0, 1], [0, 1, 0]]), 1),
          ("tie_all_trace_neg", _T(2.0 / 3.0 * np.ones((3, 3)) - np.eye(3)), 0),
          ("trace_zero", _T([[0, 0, 1], [1, 0, 0], [0, 1, 0]]), 0),
          ("identity", _T(np.eye(3)), "trace")]
    d = cs[6][1]
    assert d[0, 0] == d[1, 1] > d[2, 2]
    d = cs[7][1]
    assert d[1, 1] == d[2, 2] > d[0, 0]
    d = cs[8][1]
    assert d[0, 0] == d[1, 1] == d[2, 2] and np.trace(d[:3, :3].astype(np.float64)) <= 0
    assert np.trace(cs[9][1][:3, :3].astype(np.float64)) == 0.0
    return cs


def exp_cases():
    """(name, u[6], kind): kind 'expm' is compared with scipy's matrix exponential at 1e-12, 'small' with the
    I + Omega + Omega^2 form g2o uses below theta = 1e-5."""
    rng = np.random.default_rng(2)
    cs = [("rand%d" % k, np.concatenate([rng.uniform(-1.5, 1.5, 3), rng.uniform(-2, 2, 3)]), "expm") for k in range(20)]
    ax = np.array([0.6, -0.64, 0.48])  # unit
    ups = np.array([0.5, -0.25, 0.125])
    cs.append(("below_1e-5", np.concatenate([0.99999e-5 * ax, ups]), "small"))
    cs.append(("above_1e-5", np.concatenate([1.00001e-5 * ax, ups]), "expm"))
    cs.append(("theta_0", np.concatenate([np.zeros(3), ups]), "small"))
    for a in range(3):
        w = np.array([0.004, -0.003, 0.002])
        w[a] = np.pi - 5e-4
        cs.append(("near_pi_axis%d" % a, np.concatenate([w, [0.3, -0.7, 0.2]]), "expm"))
    return cs


def mul_cases():
    rng = np.random.default_rng(5)
    cs = []
    for k in range(12):
        a, _ = M.pose_from_cv(_T(M.rot(rng.uniform(-2, 2, 3)), rng.uniform(-3, 3, 3)))
        b, _ = M.pose_from_cv(_T(M.rot(rng.uniform(-2, 2, 3)), rng.uniform(-3, 3, 3)))
        cs.append(("rand%d" % k, a, b))
    z170 = np.array([0, 0, np.sin(np.radians(85.0)), np.cos(np.radians(85.0)), 0.2, -0.1, 0.4])
    cs.append(("w_negative", z170, z170.copy()))      # 340 degrees: the product's w is cos(170 deg) < 0 before normalizeRotation
    a, _ = M.pose_from_cv(_T(M.rot((3.1, 0.05, -0.02)), (1, 2, 3)))
    b, _ = M.pose_from_cv(_T(M.rot((0.04, 3.12, 0.03)), (-1, 0.5, 2)))
    cs.append(("two_half_turns", a, b))
    return cs


def ldlt_cases():
    """(name, H 6x6, b, lambda).  The pivot search reads the diagonal, so its order decides the exchanges."""
    cs = []
    for K in range(5):
        for Cc in range(K + 1, 6):
            H, b = M.pivot_matrix(K, Cc, 100 + 10 * K + Cc)
            cs.append(("swap_%d_%d" % (K, Cc), H, b, 0.0))
    H, b = M.pivot_matrix(0, 0, 7)
    H[np.diag_indices(6)] = [600, 500, 400, 300, 200, 100]
    cs.append(("no_exchange", H.copy(), b, 0.0))
    H[np.diag_indices(6)] = [100, 600, 500, 400, 300, 200]
    cs.append(("exchange_every_step", H.copy(), b, 0.0))
    H[np.diag_indices(6)] = 350.0
    cs.append(("equal_diagonal", H.copy(), b, 0.0))
    H[np.diag_indices(6)] = [100, 500, 500, 100, 500, 100]
    cs.append(("equal_first_wins", H.copy(), b, 0.0))
    cs.append(("indefinite", np.diag([4.0, 1.0, -2.0, 3.0, 5.0, 6.0]), np.ones(6), 0.0))
    Hz, bz = M.pivot_matrix(1, 4, 8)
    Hz[2, :] = 0.0
    Hz[:, 2] = 0.0
    cs.append(("zero_row_col", Hz, bz, 0.0))          # |d| <= DBL_MIN at the last pivot
    cs.append(("all_nan", np.full((6, 6), np.nan), np.full(6, np.nan), np.nan))   # what a NaN map point makes of H, b, lambda
    rng = np.random.default_rng(3)
    for k, lam in enumerate([0.0, 1e-3, 1.0, 1e6, 1e12]):
        Mx = rng.normal(size=(6, 6)) * rng.uniform(0.1, 100, 6)   # badly scaled, as test_oracle_ldlt_solves_and_detects_indefinite
        cs.append(("lambda_%g" % lam, Mx @ Mx.T + 1e-3 * np.eye(6), rng.normal(size=6), lam))
    return cs


CAMS = [(300.0, 900.0, 320.5, 240.25, 40.0), (900.0, 300.0, 607.1928, 185.2157, 386.1448)]
EVAL_POSES = [(0.05, -0.03, 0.02), (3.1, 0.05, -0.02), (0.04, 3.12, 0.03), (-0.03, 0.02, 3.13)]


def eval_case(n, seed, mode, pose_k, cam_k, robust):
    """An edge table of n slots seen from a camera at EVAL_POSES[pose_k]: points inside the frustum between 4 and 60 m,
    observations 0.5 px (level-scaled) off an estimate that is itself 5 cm / 0.3 degrees off the truth, a fifth of them 10 to
    40 px off (above dsqr; most of the rest below), a fifth of the slots without a map point, a tenth pre-marked outlier."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy, bf = CAMS[cam_k]
    R, t = M.rot(EVAL_POSES[pose_k]), rng.uniform(-0.5, 0.5, 3)
    z = rng.uniform(4, 60, n)
    Xc = np.stack([rng.uniform(-0.4, 0.4, n) * z, rng.uniform(-0.3, 0.3, n) * z, z], 1)
    Xw = ((Xc - t) @ R).astype(np.float32)
    lvl = rng.integers(0, 8, n)
    nz = rng.normal(0, 0.5, (n, 3)) * (1.2 ** lvl)[:, None]
    gross = rng.random(n) < 0.2
    nz[:, 0] += np.where(gross, rng.uniform(10, 40, n) * rng.choice([-1, 1], n), 0)
    u = fx * Xc[:, 0] / z + cx + nz[:, 0]
    v = fy * Xc[:, 1] / z + cy + nz[:, 1]
    ur = fx * Xc[:, 0] / z + cx - bf / z + nz[:, 2]
    mono = {"mono": np.ones(n, bool), "stereo": np.zeros(n, bool), "mixed": rng.random(n) < 0.4}[mode] | ((ur < 0) & (mode != "stereo"))
    ur = np.where(mono, -1.0, np.abs(ur)).astype(np.float32)
    keys = np.zeros(n, O.KP_DTYPE)
    keys["x"], keys["y"], keys["octave"] = u, v, lvl
    has = (rng.random(n) < 0.8).astype(np.uint8)
    outl = (rng.random(n) < 0.1).astype(np.uint8)
    if n == 1:
        has[:], outl[:] = 1, 0
    Te = _T(M.rot(np.array(EVAL_POSES[pose_k]) + [0.003, -0.002, 0.004]) , t + [0.03, -0.02, 0.05])
    pose, br = M.pose_from_cv(Te)
    return dict(n=n, keys=keys, ur=ur, has=has, Xw=Xw, outl=outl, pose=pose, branch=br, cam=CAMS[cam_k], robust=robust, mode=mode)


def eval_cases():
    cs = []
    modes = ["mixed", "mono", "stereo"]
    for k, n in enumerate([1, 15, 16, 17, 255, 256, 257, 300]):
        for r in (True, False):
            cs.append(eval_case(n, 900 + k, modes[k % 3], k % 4, k % 2, r))
    cs.append(eval_case(300, 950, "mono", 1, 0, True))
    cs.append(eval_case(300, 951, "stereo", 2, 1, True))
    cs.append(eval_case(64, 952, "mixed", 3, 0, True))
    cs.append(eval_case(64, 953, "mixed", 0, 1, False))
    return cs


_EVAL_REF = {}


def eval_refs():
    """The references of eval_cases(), computed once."""
    if not _EVAL_REF:
        cs = eval_cases()
        _EVAL_REF["cases"] = cs
        _EVAL_REF["refs"] = [M.eval_reference(c["keys"], c["ur"], c["has"], c["Xw"], c["outl"], INV_SIGMA2, c["pose"], c["cam"], c["robust"]) for c in cs]
    return _EVAL_REF["cases"], _EVAL_REF["refs"]


def eval_bound(n, mag):
    """(32 + n) * 2^-53 * sum_k |term_k|: 32 roundings per term plus the n of a summation in any order.  The terms are the
    magnitudes the roundings are relative to (pose_blocks_model.eval_reference's `mag`): for H the products
    |J[d][a] w info J[d][b]| of the three residual rows; for b and chi2 the residual e = obs - proj is itself a difference of two
    rounded numbers of a few hundred pixels, so its rounding is relative to |obs| + |proj|, not to |e| -- the terms are
    |J w info| (|obs| + |proj|) and 2 info |e| (|obs| + |proj|); the Huber weight of an edge above dsqr is delta / sqrt(chi2) and
    inherits chi2's relative error, which scales that edge's terms by 1 + (its chi2 term) / (2 chi2).  Worked out from the
    arithmetic, not from what the kernel returns."""
    return (32 + n) * 2.0 ** -53 * mag


# ================================================================ CPU: the references against the oracle's hooks

def test_model_quaternion_matches_oracle_on_the_gpu_cases():
    L = _hooks()
    seen = set()
    for name, T, want in from_cv_cases():
        R = np.ascontiguousarray(T[:3, :3].astype(np.float64))
        q = np.zeros(4); Ro = np.zeros(9)
        L.orc_test_quat_roundtrip(R.ctypes.data, q.ctypes.data, Ro.ctypes.data)
        pose, br = M.pose_from_cv(T)
        seen.add(br)
        if want is not None:
            assert br == want, name
        assert np.abs(pose[:4] - q).max() <= 1e-15, name            # same operations in the same order
        assert np.array_equal(M.pose_to_cv(pose)[:3, :3].astype(np.float64), Ro.reshape(3, 3)), name
        assert np.abs(Ro.reshape(3, 3) - R).max() < 2e-7, name
    assert seen == {"trace", 0, 1, 2}


def test_model_exp_matches_oracle_on_the_gpu_cases():
    L = _hooks()
    for name, u, kind in exp_cases():
        u = np.ascontiguousarray(u)
        T = np.zeros(12)
        L.orc_test_se3_exp(u.ctypes.data, T.ctypes.data)
        ref = M.se3_exp_matrix(u)[:3] if kind == "expm" else M.pose_to_matrix(M.se3_exp_small(u))[:3]
        assert np.abs(T.reshape(3, 4) - ref).max() < 1e-12, name
    # the two forms differ by half of Omega upsilon just below the threshold: the 'small' reference is not expm
    u = exp_cases()[20][1]
    assert np.abs(M.pose_to_matrix(M.se3_exp_small(u))[:3, 3] - M.se3_exp_matrix(u)[:3, 3]).max() > 1e-7


def test_model_mul_matches_matrix_products():
    """No oracle hook takes two poses; the quaternion reference is checked against 4x4 products, the test of the GPU test."""
    for name, a, b in mul_cases():
        r = M.se3_mul(a, b)
        assert abs(np.linalg.norm(r[:4]) - 1) < 1e-15 and r[3] >= 0, name
        assert np.abs(M.pose_to_matrix(r) - M.pose_to_matrix(a) @ M.pose_to_matrix(b)).max() < 1e-14 * 6, name
    a, b = mul_cases()[12][1:]
    assert a[3] * b[3] - a[:3] @ b[:3] < 0


def test_model_ldlt_matches_oracle_and_reaches_every_exchange():
    L = _hooks()
    seen = set()
    for name, H, b, lam in ldlt_cases():
        x, positive, piv = M.ldlt_solve(H, b, lam)
        seen |= M.exchanges(piv)
        Hl = np.ascontiguousarray(np.asarray(H, np.float64) + lam * np.eye(6)); bb = np.ascontiguousarray(b, np.float64); xo = np.full(6, 7.0)
        assert L.orc_test_ldlt6(Hl.ctypes.data, bb.ctypes.data, xo.ctypes.data) == int(positive), name
        if positive:
            assert np.array_equal(x, xo), name                      # same operations in the same order
        else:
            assert (xo == 7.0).all(), name
        if name.startswith("swap_"):
            K, Cc = int(name[5]), int(name[7])
            assert piv[K] == (K, Cc) and all(p == k for k, p in piv[:K]), (name, piv)
    assert seen == {(k, c) for k in range(5) for c in range(k + 1, 6)}
    by = {c[0]: M.ldlt_solve(c[1], c[2], c[3]) for c in ldlt_cases()}
    assert M.exchanges(by["no_exchange"][2]) == set() and M.exchanges(by["equal_diagonal"][2]) == set()
    assert len(M.exchanges(by["exchange_every_step"][2])) == 5
    assert by["equal_first_wins"][2][0] == (0, 1)
    assert by["indefinite"][1] is False
    assert by["zero_row_col"][1] is True and by["zero_row_col"][0][2] == 0.0
    assert by["all_nan"][1] is True and (by["all_nan"][0] == 0.0).all()   # NaN > DBL_MIN is false: every quotient is replaced by 0


def test_model_eval_matches_a_plain_float64_sum():
    """eval_reference against an independent dense restatement (numpy float64, J^T W J by matrix products) on one mixed case:
    the two agree to float64 rounding, and the case has edges on both sides of dsqr, holes and pre-marked outliers."""
    c = eval_case(64, 952, "mixed", 3, 0, True)
    tot, mag = M.eval_reference(c["keys"], c["ur"], c["has"], c["Xw"], c["outl"], INV_SIGMA2, c["pose"], c["cam"], True)
    fx, fy, cx, cy, bf = c["cam"]
    R, t = M.quat_to_matrix(c["pose"]), c["pose"][4:7]
    H = np.zeros((6, 6)); b = np.zeros(6); chi_t = 0.0; cnt = 0; above = below = 0
    for i in range(c["n"]):
        if not c["has"][i] or c["outl"][i]:
            continue
        x, y, z = R @ c["Xw"][i].astype(np.float64) + t
        st = c["ur"][i] >= 0
        info = float(INV_SIGMA2[c["keys"]["octave"][i]])
        iz = float(np.float32(1 / z)) if st else 1 / z
        pr = [x * iz * fx + cx, y * iz * fy + cy]
        ob = [float(c["keys"]["x"][i]), float(c["keys"]["y"][i])]
        J = [[x * y / z**2 * fx, -(1 + x * x / z**2) * fx, y / z * fx, -fx / z, 0, x / z**2 * fx],
             [(1 + y * y / z**2) * fy, -x * y / z**2 * fy, -x / z * fy, 0, -fy / z, y / z**2 * fy]]
        if st:
            pr.append(pr[0] - bf * iz); ob.append(float(c["ur"][i]))
            J.append([J[0][0] - bf * y / z**2, J[0][1] + bf * x / z**2, J[0][2], J[0][3], 0, J[0][5] - bf / z**2])
        J = np.array(J); e = np.array(ob) - np.array(pr)
        chi = info * float(e @ e)
        d = M.DELTA_STEREO if st else M.DELTA_MONO
        w = 1.0
        if chi > d * d:
            above += 1; w = d / np.sqrt(chi); chi_t += 2 * np.sqrt(chi) * d - d * d
        else:
            below += 1; chi_t += chi
        H += J.T @ J * (w * info); b -= J.T @ e * (w * info); cnt += 1
    assert above >= 3 and below >= 10 and cnt < c["n"] - 5
    got = np.concatenate([H[np.triu_indices(6)], b, [chi_t, cnt]])
    assert np.abs(got - tot).max() <= 1e-9 * np.abs(tot).max()
    assert np.all(np.abs(got - tot) <= 1e3 * eval_bound(c["n"], mag) + 1e-300)
    assert tot[28] == cnt and (np.delete(mag[:28], 16) > 0).all()
    assert tot[16] == 0.0 and mag[16] == 0.0   # H[3][4]: no residual row has both entries, the total must be an exact zero


def test_eval_cases_cover_what_the_issue_lists():
    cs, refs = eval_refs()
    assert {c["n"] for c in cs} >= {1, 15, 16, 17, 255, 256, 257, 300}
    assert {c["mode"] for c in cs} == {"mono", "stereo", "mixed"} and {c["branch"] for c in cs} == {"trace", 0, 1, 2}
    assert {c["cam"] for c in cs} == set(CAMS) and {c["robust"] for c in cs} == {True, False}
    assert any((c["has"] == 0).any() for c in cs) and any((c["outl"] != 0).any() for c in cs)
    assert any(((c["ur"] >= 0) & (c["has"] > 0)).any() and ((c["ur"] < 0) & (c["has"] > 0)).any() for c in cs)


# ================================================================ GPU: the blocks against the references

@pytest.mark.gpu
def test_gpu_from_cv_and_to_cv_all_branches_and_ties():
    cs = from_cv_cases()
    out = _run(OP_FROM_CV, [c[1].reshape(16).astype(np.float64) for c in cs])
    for (name, T, want), o in zip(cs, out):
        pose, br = M.pose_from_cv(T)
        q = o[:4]
        assert abs(np.linalg.norm(q) - 1) < 1e-14 and q[3] >= 0, name
        # a wrong branch gives the same rotation only up to rounding, and at the ties a different quaternion altogether
        assert np.abs(o[:7] - pose).max() <= 1e-14, (name, br, o[:7], pose)
        back = o[7:].reshape(4, 4)
        assert np.abs(back - T.astype(np.float64)).max() < 2e-7, name
        assert np.array_equal(back[3], [0, 0, 0, 1])


@pytest.mark.gpu
def test_gpu_se3_exp_against_expm_and_the_small_angle_form():
    cs = exp_cases()
    out = _run(OP_EXP, [c[1] for c in cs])
    for (name, u, kind), o in zip(cs, out):
        assert abs(np.linalg.norm(o[:4]) - 1) < 1e-14 and o[3] >= 0, name
        if kind == "expm":
            assert np.abs(M.pose_to_matrix(o)[:3] - M.se3_exp_matrix(u)[:3]).max() < 1e-12, name
        else:
            assert np.abs(o - M.se3_exp_small(u)).max() <= 1e-14, name
        if name.startswith("near_pi"):
            assert M.quat_branch(M.pose_to_matrix(o)[:3, :3]) == int(name[-1]), name   # the rotation lands in a non-trace branch


@pytest.mark.gpu
def test_gpu_se3_mul_against_matrix_products():
    cs = mul_cases()
    out = _run(OP_MUL, [np.concatenate([a, b]) for _, a, b in cs])
    for (name, a, b), o in zip(cs, out):
        assert abs(np.linalg.norm(o[:4]) - 1) < 1e-14 and o[3] >= 0, name
        ref = M.pose_to_matrix(a) @ M.pose_to_matrix(b)
        # entries of R are <= 1, |t| <= 6 here: a few roundings of 2^-53 * 6
        assert np.abs(M.pose_to_matrix(o) - ref).max() < 1e-14 * 6, name
        assert np.abs(o - M.se3_mul(a, b)).max() < 1e-14 * 6, name
    a, b = cs[12][1], cs[12][2]
    assert a[3] * b[3] - a[:3] @ b[:3] < 0   # the case whose raw w is negative


@pytest.mark.gpu
def test_gpu_ldlt_every_exchange_and_the_edge_cases():
    cs = ldlt_cases()
    out = _run(OP_LDLT, [np.concatenate([M.pack_system(H, b), [lam]]) for _, H, b, lam in cs])
    seen = set()
    for (name, H, b, lam), o in zip(cs, out):
        x, positive, piv = M.ldlt_solve(H, b, lam)
        seen |= M.exchanges(piv)
        assert o[6] == float(positive), name
        if not positive:
            assert (o[:6] == 7.0).all(), name                       # x untouched
            continue
        if name in ("zero_row_col", "all_nan"):                     # singular: the answer is the oracle's rule, not linalg.solve's
            assert np.abs(o[:6] - x).max() <= 1e-12 * max(1.0, np.abs(x).max()), (name, o[:6], x)
            continue
        Hl = np.asarray(H, np.float64) + lam * np.eye(6)
        ref = np.linalg.solve(Hl, b)
        assert np.abs(o[:6] - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max()) * np.linalg.cond(Hl) * 1e-3 + 1e-12, name
    assert seen == {(k, c) for k in range(5) for c in range(k + 1, 6)}


@pytest.mark.gpu
def test_gpu_eval_pass_totals_against_the_reference():
    cs, refs = eval_refs()
    off = np.cumsum([0] + [c["n"] for c in cs])
    hdr = np.zeros((len(cs), 16))
    for k, c in enumerate(cs):
        hdr[k, 0], hdr[k, 1], hdr[k, 2:9], hdr[k, 9:14], hdr[k, 15] = c["n"], float(c["robust"]), c["pose"], c["cam"], off[k]
    cat = {f: np.ascontiguousarray(np.concatenate([c[f] for c in cs])) for f in ("keys", "ur", "has", "Xw", "outl")}
    sig = np.ascontiguousarray(INV_SIGMA2)
    arg = _EvalIn(hdr.ctypes.data, cat["keys"].ctypes.data, cat["ur"].ctypes.data, cat["has"].ctypes.data, cat["Xw"].ctypes.data,
                  cat["outl"].ctypes.data, sig.ctypes.data, int(off[-1]))
    out = np.zeros((len(cs), 62))
    assert _lib().pose_blocks_run(OP_EVAL, len(cs), C.addressof(arg), out.ctypes.data) == 0
    worst = 0.0
    for k, (c, (tot, mag)) in enumerate(zip(cs, refs)):
        lds, hbm = out[k, :29], out[k, 29:58]
        assert np.array_equal(lds, hbm), k                          # the two instances agree bit for bit
        assert out[k, 58] == lds[27] and out[k, 59] == lds[28] and out[k, 60] == lds[27] and out[k, 61] == lds[28]
        assert lds[28] == tot[28], k
        bound = eval_bound(c["n"], mag)
        ratio = np.abs(lds[:28] - tot[:28]) / np.where(bound[:28] > 0, bound[:28], 1.0)
        print("eval case %2d n=%3d %-6s robust=%d branch=%-5s active=%3d  max ratio to bound %.4f (total %d)"
              % (k, c["n"], c["mode"], c["robust"], c["branch"], int(tot[28]), ratio.max(), int(ratio.argmax())))
        worst = max(worst, float(ratio.max()))
        assert (np.abs(lds[:28] - tot[:28]) <= bound[:28]).all(), (k, int(ratio.argmax()), float(ratio.max()))
    print("eval: largest ratio to the bound %.4f" % worst)
