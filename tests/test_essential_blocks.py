"""The device building blocks of OptimizeEssentialGraph (orbslam2_amd/csrc/orbfe_essential_blocks.hpp) one at a time, through the test-only
tests/essential_blocks/essential_blocks.hip, against the float64 model (tests/essential_graph_model.py): Sim3::log per branch, one edge's
error and both numeric Jacobians (free-free and free-fixed, fix_scale on and off), the assembly of a 3-vertex system, the block LDLT alone
on a planned ring (workspace in the LDS and in HBM), and the recovery / point stage bit for bit.

Bounds.  log and the error: the model calls glibc's log / acos / sin / cos, the device its own; a few ulp each on values below 4, through
a 3 x 3 solve of condition below 10: LOG_ATOL = 1e-13.  The Jacobians: both sides are quotients of rounding noise by 2e-9, the bound is the
one tests/test_essential_graph_model.py derives (2 x 32 roundings x eps x 4 / 2e-9).  The assembly from GIVEN edge blocks repeats the
model's products in another association (numpy's matmul): sums of 7 products per edge, relative to the largest entry ASM_RTOL = 64 eps.
The evaluation pass (device edge blocks, device assembly) inherits the Jacobians' noise: measured on the MI355X, bound 8 x the maximum
rounded up to one digit (EVAL_H_RTOL, EVAL_B_RTOL; DESIGN.md section 4s has both columns).  The LDLT: 1e-12 relative against
numpy.linalg.solve, as the plan's numpy run is held to."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import essential_graph_model as M
from tests import essential_graph_scenes as SC
from tests import sim3_opt_model as S3

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = np.finfo(np.float64).eps
LOG_ATOL = 1e-13
JAC_ATOL = 2 * 32 * EPS * 4 / 2e-9
ASM_RTOL = 64 * EPS
EVAL_H_RTOL = 2e-9   # measured 1.692e-10
EVAL_B_RTOL = 7e-10  # measured 8.060e-11


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(HERE, "essential_blocks", "libessential_blocks.so")
    if not os.path.exists(path):
        pytest.fail("tests/essential_blocks/libessential_blocks.so is not built (run build())")
    import torch  # noqa: F401  (its HIP runtime first, as orbslam2_amd.api.load does)
    L = C.CDLL(path)
    for f in ("eb_log", "eb_edge", "eb_assemble", "eb_solve", "eb_finish"):
        getattr(L, f).restype = C.c_int
    L.eb_log.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    L.eb_edge.argtypes = [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p]
    L.eb_assemble.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.eb_solve.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_void_p, C.c_void_p]
    L.eb_finish.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def p(a):
    return a.ctypes.data_as(C.c_void_p)


AX = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])


@pytest.mark.gpu
def test_log_in_every_branch(lib):
    cases = []
    for sigma in (0.0, 0.9e-5, -1.1e-5, 0.3, -0.2):
        for theta in (0.0, 1e-7, 1e-3, 4.4e-3, 4.6e-3, 0.5, 3.0):
            if abs(sigma) >= 1e-5 and 0 < theta < 4.5e-3:
                continue   # g2o's B there is 1 / sigma^3: a condition number, not a branch to compare ulps in (theta == 0 covers the branch)
            cases.append(S3.sim3_exp(list(theta * AX) + [0.4, -0.7, 0.2, sigma]))
    sc = SC.closed_ring(6)
    P = M.Problem(**{k: sc[k] for k in ("Tcw", "fixed_kf", "edge_i", "edge_j", "edge_kind", "corrected", "has_corrected", "noncorrected", "has_noncorrected")})
    for e in P.active():   # and what the kernel really takes the logarithm of
        i, j = P.edges[e]
        cases.append(S3.sim3_mul(S3.sim3_mul(P.meas[e], P.init[i]), S3.sim3_inverse(P.init[j])))
    assert {M.log_branch(S) for S in cases} == {(a, b) for a in (True, False) for b in (True, False)}
    S = np.array([S3.pack(x) for x in cases])
    out = np.zeros((len(cases), 7))
    assert lib.eb_log(len(cases), p(S), p(out)) == 0
    want = np.array([M.sim3_log(x) for x in cases])
    d = np.abs(out - want).max()
    print("\nlog: largest |device - model| = %.3e over %d cases" % (d, len(cases)))
    assert d <= LOG_ATOL


def _edge(lib, C8, Si, Sj, free_i, free_j, fix_scale):
    out = np.zeros(105)
    a, b, c = (np.ascontiguousarray(S3.pack(x)) for x in (C8, Si, Sj))
    assert lib.eb_edge(p(a), p(b), p(c), int(free_i), int(free_j), int(fix_scale), p(out)) == 0
    return out[:7], out[7:56].reshape(7, 7), out[56:].reshape(7, 7)


@pytest.mark.gpu
@pytest.mark.parametrize("fix_scale", [False, True])
@pytest.mark.parametrize("free_j", [True, False])
def test_edge_error_and_jacobians(lib, fix_scale, free_j):
    sc = SC.closed_ring(6)
    P = M.Problem(**{k: sc[k] for k in ("Tcw", "fixed_kf", "edge_i", "edge_j", "edge_kind", "corrected", "has_corrected", "noncorrected", "has_noncorrected")})
    worst = [0.0, 0.0]
    for e in P.active():
        i, j = P.edges[e]
        err, Ji, Jj = _edge(lib, P.meas[e], P.init[i], P.init[j], True, free_j, fix_scale)
        werr, wJi, wJj = M.edge_linearize(P.meas[e], M.perturbed(P.init[i], fix_scale), M.perturbed(P.init[j], fix_scale), True, free_j)
        worst = [max(worst[0], np.abs(err - werr).max()), max(worst[1], np.abs(Ji - wJi).max(), np.abs(Jj - wJj).max())]
        if not free_j:
            assert not Jj.any()       # no block for a fixed vertex
        if fix_scale:
            assert not Ji[:, 6].any() and not Jj[:, 6].any()
        else:
            assert Ji[:, 6].any()
    print("\nedge (fix_scale %d, free_j %d): error %.3e, Jacobians %.3e" % (fix_scale, free_j, worst[0], worst[1]))
    assert worst[0] <= LOG_ATOL and worst[1] <= JAC_ATOL


def _three_vertex_problem():
    sc = SC.closed_ring(4, n_corrected=2)
    P = M.Problem(**{k: sc[k] for k in ("Tcw", "fixed_kf", "edge_i", "edge_j", "edge_kind", "corrected", "has_corrected", "noncorrected", "has_noncorrected")})
    return sc, P


@pytest.mark.gpu
def test_assembly_of_a_three_vertex_system(lib):
    from orbslam2_amd import api
    sc, P = _three_vertex_problem()
    blob = np.ascontiguousarray(api.essential_graph_plan(4, 0, sc["edge_i"], sc["edge_j"]))
    plan = M.parse_plan(blob)
    assert plan["n_free"] == 3
    _, _, _, blocks = P.linearize(P.init, False)
    n_edges = len(P.edges)
    # (a) from the model's edge blocks: the assembly alone
    flat = np.zeros((n_edges, 105))
    for e, (err, Ji, Jj) in blocks.items():
        flat[e] = np.concatenate([err, Ji.reshape(-1), Jj.reshape(-1)])
    H, b = np.zeros((plan["n_slots"], 49)), np.zeros((3, 7))
    assert lib.eb_assemble(p(blob), len(blob), p(flat), n_edges, p(H), p(b)) == 0
    wH, wb = M.plan_assemble(plan, blocks)
    dH, db = np.abs(H.reshape(-1, 7, 7) - wH).max() / np.abs(wH).max(), np.abs(b - wb).max() / np.abs(wb).max()
    print("\nassembly alone: H %.3e b %.3e (relative to the largest entry)" % (dH, db))
    assert dH <= ASM_RTOL and db <= ASM_RTOL
    # (b) the evaluation pass: the device's own edge blocks, then the device's assembly
    dev = np.zeros((n_edges, 105))
    for e in P.active():
        i, j = P.edges[e]
        err, Ji, Jj = _edge(lib, P.meas[e], P.init[i], P.init[j], i != 0, j != 0, False)
        dev[e] = np.concatenate([err, Ji.reshape(-1), Jj.reshape(-1)])
    assert lib.eb_assemble(p(blob), len(blob), p(dev), n_edges, p(H), p(b)) == 0
    dH, db = np.abs(H.reshape(-1, 7, 7) - wH).max() / np.abs(wH).max(), np.abs(b - wb).max() / np.abs(wb).max()
    print("evaluation pass: H %.3e b %.3e (relative to the largest entry)" % (dH, db))
    assert dH <= EVAL_H_RTOL and db <= EVAL_B_RTOL
    # the slots are the dense edge-sequential system, permuted
    Hd, bd, _, _ = P.linearize(P.init, False)
    perm = np.concatenate([7 * P.col[int(v)] + np.arange(7) for v in plan["order"]])
    A = M.plan_dense(plan, H.reshape(-1, 7, 7))
    assert np.abs(A - Hd[np.ix_(perm, perm)]).max() <= EVAL_H_RTOL * np.abs(Hd).max()


@pytest.mark.gpu
@pytest.mark.parametrize("graph", ["ring6", "ring8_chord"])
def test_block_ldlt_alone_in_lds_and_in_hbm(lib, graph):
    from orbslam2_amd import api
    from tests.test_essential_graph_plan import GRAPHS, usable
    n, fixed, edges = GRAPHS[graph]
    blob = np.ascontiguousarray(api.essential_graph_plan(n, fixed, [e[0] for e in edges], [e[1] for e in edges]))
    plan = M.parse_plan(blob)
    rng = np.random.default_rng(5)
    blocks = {}
    for e, (i, j) in enumerate(edges):
        if usable(n, i, j):
            Ji, Jj = (np.eye(7) * rng.uniform(1, 2) + 0.2 * rng.normal(size=(7, 7)) for _ in range(2))
            blocks[e] = (rng.normal(size=7), Ji if i != fixed else np.zeros((7, 7)), Jj if j != fixed else np.zeros((7, 7)))
    Hs, b = M.plan_assemble(plan, blocks)
    lam = 1e-3
    want = np.linalg.solve(M.plan_dense(plan, Hs) + lam * np.eye(7 * (n - 1)), b.reshape(-1))
    xs = []
    for in_lds in (1, 0):
        x, ok = np.zeros(7 * (n - 1)), np.zeros(1, np.int32)
        assert lib.eb_solve(p(blob), len(blob), p(np.ascontiguousarray(Hs)), p(np.ascontiguousarray(b)), lam, in_lds, p(x), p(ok)) == 0
        assert ok[0] == 1
        assert np.abs(x - want).max() <= 1e-12 * np.abs(want).max()
        assert np.abs(x - M.plan_solve(plan, Hs, b, lam).reshape(-1)).max() <= 1e-12 * np.abs(want).max()
        xs.append(x)
    assert xs[0].tobytes() == xs[1].tobytes()   # the same arithmetic wherever the workspace lies
    # a zero pivot is a failed factorisation, reported and survived
    Hz = np.zeros_like(Hs)
    x, ok = np.zeros(7 * (n - 1)), np.ones(1, np.int32)
    assert lib.eb_solve(p(blob), len(blob), p(Hz), p(np.ascontiguousarray(b)), 0.0, 1, p(x), p(ok)) == 0
    assert ok[0] == 0


@pytest.mark.gpu
def test_recovery_and_point_correction_bit_for_bit(lib):
    out = M.run(**SC.scene("ring6"))
    final = [S3.unpack(v) for v in out["sim3"]]
    S = np.ascontiguousarray(out["sim3"])
    n = len(final)
    T, Ow = np.zeros((n, 16), np.float32), np.zeros((n, 3), np.float32)
    rng = np.random.default_rng(3)
    pos = rng.uniform(-5, 5, (40, 3)).astype(np.float32)
    ref = rng.integers(0, n, 40)
    P = out["problem"]
    Srw = np.ascontiguousarray([S3.pack(P.init[r]) for r in ref])
    Swr = np.ascontiguousarray([S3.pack(S3.sim3_inverse(final[r])) for r in ref])
    got = pos.copy()
    assert lib.eb_finish(n, p(S), p(T), p(Ow), 40, p(Srw), p(Swr), p(got)) == 0
    for v in range(n):
        wT, wOw = M.recover_pose(final[v])
        assert T[v].tobytes() == wT.tobytes() and Ow[v].tobytes() == wOw.tobytes()
    for q in range(40):
        assert got[q].tobytes() == M.correct_point(P.init[ref[q]], S3.sim3_inverse(final[ref[q]]), pos[q]).tobytes()
