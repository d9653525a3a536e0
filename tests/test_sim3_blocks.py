"""The device blocks of OptimizeSim3 (orbslam2_amd/csrc/orbfe_sim3_blocks.hpp, and solve_ldlt<7> of orbfe_pose_blocks.hpp), one at a time,
against the float64 model (tests/sim3_opt_model.py) on the case lists of tests/sim3_opt_scenes.py -- the cases on which
tests/test_sim3_opt_model.py has proven the model on the CPU.  tests/sim3_blocks/sim3_blocks.hip (test-only, the product's compiler flags)
runs sim3_from_rts, sim3_exp, sim3_mul, sim3_inverse, sim3_map, solve_ldlt<7> and one sim3_eval_pass alone.

Why the evaluation pass is compared entry by entry: Levenberg reaches the same optimum with a wrong off-diagonal of H as long as b and
chi2 are right, so the whole-call test (tests/test_sim3_opt_device.py) cannot see one.  All 28 entries of H, all 7 of b, chi2 and the
count are compared here.

EVAL_RTOL -- H and b come from g2o's numeric Jacobian: each entry of J carries the rounding noise of two error evaluations divided by
2e-9 (about 1e-6 of J; tests/test_sim3_opt_model.py bounds it), and the device's roundings differ from the model's (fused multiply-adds,
another summation order).  The bound is therefore measured, as the issue of this feature prescribes: the largest
|device - model| over all eval cases on the MI355X, relative to the largest |H| entry for H and to the largest entry of
sum |J|^T w |e| for b, was  H 5.1e-08 (case n16), b 3.0e-08 (case n1);  EVAL_RTOL = 8 x 5.1e-08 = 4.1e-07, rounded up to one digit: 5e-07.
The small cases are the noisiest: with few edges the noise of single Jacobian entries does not average out.
chi2 does not pass through J: its bound is worked out from the arithmetic ((64 + n) roundings of the terms' magnitudes).
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import sim3_opt_model as M
from tests import sim3_opt_scenes as S

HERE = os.path.dirname(os.path.abspath(__file__))
OP_FROM_RTS, OP_EXP, OP_MUL, OP_INVERSE, OP_MAP, OP_LDLT7, OP_EVAL = 1, 2, 3, 4, 5, 6, 7
IN_STRIDE = {OP_FROM_RTS: 13, OP_EXP: 7, OP_MUL: 16, OP_INVERSE: 8, OP_MAP: 11, OP_LDLT7: 36}
OUT_STRIDE = {OP_FROM_RTS: 8, OP_EXP: 8, OP_MUL: 8, OP_INVERSE: 8, OP_MAP: 3, OP_LDLT7: 8, OP_EVAL: 39}
EVAL_RTOL = 5e-7   # see the header: 8 x the measured 5.1e-08, rounded up to one digit


class _EvalIn(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("hdr", "rows", "active")] + [("total", C.c_int32)]


def _lib():
    path = os.path.join(HERE, "sim3_blocks", "libsim3_blocks.so")
    if not os.path.exists(path):
        raise RuntimeError("tests/sim3_blocks/libsim3_blocks.so is missing: __graft_entry__.build() compiles it")
    L = C.CDLL(path)
    L.sim3_blocks_run.restype = C.c_int
    L.sim3_blocks_run.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return L


def _run(op, cases):
    a = np.ascontiguousarray(cases, np.float64).reshape(-1, IN_STRIDE[op])
    out = np.zeros((len(a), OUT_STRIDE[op]))
    assert _lib().sim3_blocks_run(op, len(a), a.ctypes.data, out.ctypes.data) == 0
    return out


def test_the_blocks_library_is_built_by_build():
    """CPU: build() names the library's Makefile, and the Makefile uses the product's flags."""
    root = os.path.dirname(HERE)
    assert 'os.path.join(ROOT, "tests", "sim3_blocks")' in open(os.path.join(root, "__graft_entry__.py")).read()
    flags = lambda p: [l for l in open(p).read().split("\n") if l.startswith("FLAGS") or l.startswith("          -f")]
    assert flags(os.path.join(HERE, "sim3_blocks", "Makefile")) == flags(os.path.join(HERE, "pose_blocks", "Makefile"))


@pytest.mark.gpu
def test_gpu_sim3_from_rotation_translation_scale():
    cs = S.rts_cases()
    out = _run(OP_FROM_RTS, [np.concatenate([np.asarray(R, np.float64).reshape(9), t, [s]]) for _, R, t, s, _ in cs])
    for (name, R, t, s, br), o in zip(cs, out):
        # the same operations in the same order (a square root, a division, sums of two): a wrong branch differs in the first digits
        assert np.abs(o - M.pack(M.sim3(R, t, s))).max() <= 1e-15, (name, br)
    assert abs(np.linalg.norm(out[-1][:4]) - 1) > 1e-13   # not normalised


@pytest.mark.gpu
def test_gpu_exponential_in_four_branches():
    from scipy.linalg import expm
    from tests.test_sim3_opt_model import _generator
    cs = S.exp_cases()
    out = _run(OP_EXP, [c[1] for c in cs])
    for (name, u, branch, kind), o in zip(cs, out):
        ref = M.pack(M.sim3_exp(u))
        # Entries are O(1); sin, cos and exp of the device library and of libm differ in the last bits: 1e-14.  The closed forms cancel
        # next to their thresholds: 1 - cos(theta) carries a last-bit error of 1.0, so A = (1 - cos theta) / theta^2 one of
        # 2^-53 / theta^2, which reaches t through A Omega upsilon (theta |upsilon|); s - 1 likewise, so C = (s - 1) / sigma one of
        # 2^-53 / |sigma|, which reaches t through C upsilon and through B Omega^2 upsilon (B holds C / theta^2).  Four last bits each.
        theta, sigma, ups = np.linalg.norm(u[:3]), abs(u[6]), np.linalg.norm(u[3:6])
        tol = 1e-14 + 4 * 2.0 ** -53 * ups * ((1 / theta if theta >= 1e-5 else 0.0) + (2 / sigma if sigma >= 1e-5 else 0.0))
        assert np.abs(o - ref).max() <= tol, (name, np.abs(o - ref).max(), tol)
        if kind == "expm":
            q = o[:4] / np.linalg.norm(o[:4])
            assert np.abs(M.sim3_matrix((tuple(q), tuple(o[4:7]), o[7])) - expm(_generator(u))).max() < 1e-12, name
    by = {c[0]: o for c, o in zip(cs, out)}
    assert abs(np.linalg.norm(by["theta_below"][:4]) - 1) > 1e-11   # R = I + Omega + Omega^2 went to Quaterniond(R) as it is


@pytest.mark.gpu
def test_gpu_product_inverse_and_map():
    cs = S.sim3_cases()
    mul = _run(OP_MUL, [np.concatenate([a, b]) for _, a, b, _ in cs])
    inv = _run(OP_INVERSE, [a for _, a, _, _ in cs])
    mp = _run(OP_MAP, [np.concatenate([a, p]) for _, a, _, p in cs])
    for (name, a, b, p), om, oi, op in zip(cs, mul, inv, mp):
        A, B = M.unpack(a), M.unpack(b)
        # entries are below 16 (|t| <= 3, s <= 2, |p| <= 9): 16 roundings of 2^-53 * 16 = 2.8e-14
        assert np.abs(om - M.pack(M.sim3_mul(A, B))).max() < 3e-14, name
        assert np.abs(oi - M.pack(M.sim3_inverse(A))).max() < 3e-14, name
        assert np.abs(op - np.array(M.sim3_map(A, *p))).max() < 3e-14, name
        assert abs(np.linalg.norm(om[:4]) - np.linalg.norm(a[:4]) * np.linalg.norm(b[:4])) < 1e-14   # the product is not normalised


@pytest.mark.gpu
def test_gpu_ldlt7_every_exchange_and_the_edge_cases():
    cs = S.ldlt7_cases()
    out = _run(OP_LDLT7, [np.concatenate([np.asarray(H, np.float64)[np.triu_indices(7)], b, [lam]]) for _, H, b, lam in cs])
    seen = set()
    for (name, H, b, lam), o in zip(cs, out):
        x, positive, piv = M.ldlt_solve(H, b, lam)
        seen |= {(k, p) for k, p in piv if p != k}
        assert o[7] == float(positive), name
        if not positive:
            assert (o[:7] == 7.0).all(), name                       # x untouched
            continue
        if name == "zero_row_col":                                  # singular: the answer is the model's rule, not linalg.solve's
            assert np.abs(o[:7] - x).max() <= 1e-12 * max(1.0, np.abs(x).max()), name
            assert o[2] == 0.0
            continue
        Hl = np.asarray(H, np.float64) + lam * np.eye(7)
        ref = np.linalg.solve(Hl, b)
        assert np.abs(o[:7] - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max()) * np.linalg.cond(Hl) * 1e-3 + 1e-12, name
        if name == "fix_scale":
            assert o[6] == 0.0                                      # b[6] = 0 over lambda alone
    assert seen == {(k, c) for k in range(6) for c in range(k + 1, 7)}


@pytest.mark.gpu
def test_gpu_eval_pass_every_entry_against_the_model():
    cs, refs = S.eval_refs()
    off = np.cumsum([0] + [len(c[1]) for c in cs])
    delta = float(np.float32(np.sqrt(np.float32(S.TH2))))
    hdr = np.zeros((len(cs), 16))
    rows, act = [], []
    for k, (name, T, est, fix) in enumerate(cs):
        hdr[k, 0], hdr[k, 1], hdr[k, 2:10], hdr[k, 10:14], hdr[k, 14], hdr[k, 15] = len(T), float(fix), M.pack(est), S.CAM, delta, off[k]
        r = np.concatenate([T.P1, T.P2, T.obs1, T.obs2, T.info1[:, None], T.info2[:, None]], 1)
        assert np.array_equal(r.astype(np.float32).astype(np.float64), r)   # the table holds floats: nothing is lost
        rows.append(r.astype(np.float32)); act.append(T.active.astype(np.uint8))
    rows, act = np.ascontiguousarray(np.concatenate(rows)), np.ascontiguousarray(np.concatenate(act))
    arg = _EvalIn(hdr.ctypes.data, rows.ctypes.data, act.ctypes.data, int(off[-1]))
    out = np.zeros((len(cs), 39))
    assert _lib().sim3_blocks_run(OP_EVAL, len(cs), C.addressof(arg), out.ctypes.data) == 0
    worst_H = worst_b = 0.0
    iu = np.triu_indices(7)
    for k, ((name, T, est, fix), (H, b, chi, cnt, magH, magb, magc)) in enumerate(zip(cs, refs)):
        o = out[k]
        assert o[36] == cnt == o[38] and o[37] == o[35], name
        eH, eb = np.abs(o[:28] - H[iu]).max() / magH, np.abs(o[28:35] - b).max() / magb
        print("eval case %-8s n=%3d active=%3d fix=%d  H %.3e  b %.3e  chi2 %.3e (rel)" % (name, len(T), cnt, fix, eH, eb, abs(o[35] - chi) / chi))
        worst_H, worst_b = max(worst_H, eH), max(worst_b, eb)
        assert abs(o[35] - chi) <= (64 + len(T)) * 2.0 ** -53 * magc, name
        if fix:                                                     # column 6 of every Jacobian is exactly zero
            assert (o[[6, 12, 17, 21, 24, 26, 27]] == 0).all() and o[34] == 0, name
    print("eval: largest |device - model|: H %.3e of max|H|, b %.3e of max sum|J|w|e|" % (worst_H, worst_b))
    for k, ((name, T, est, fix), (H, b, chi, cnt, magH, magb, magc)) in enumerate(zip(cs, refs)):
        assert np.abs(out[k, :28] - H[iu]).max() <= EVAL_RTOL * magH, name
        assert np.abs(out[k, 28:35] - b).max() <= EVAL_RTOL * magb, name
