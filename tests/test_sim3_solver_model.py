"""The model of the Sim3Solver port (tests/sim3_solver_model.py) proven on the CPU: known answers, the truncated gates, the coincident
triple, the comparison with a float64 path shaped like the reference (np.linalg.eigh, the angle-axis of src/Sim3Solver.cc:275-285,
Rodrigues) and Sim3Solver::iterate against its literal transcription.  tests/test_sim3_solver_host.py compares the host form and
tests/test_sim3_ransac_device.py the kernels with this model bit for bit.

The float64 comparison: on the random scenes (40 correspondences, 30 inliers, 300 hypotheses: 12 000 cases each) every inlier / outlier
classification equals the float64 path's; the only cases left out are those whose float64 error lies within a relative 1e-3 of its
gate, and they may be at most 0.1 % of all cases.  Measured on this file's scenes: 2, 3 and 1 of 12 000 left out, no disagreement
outside them; the largest |R, t, s - float64 path| is 3.5e-05 (recorded in DESIGN.md section 4o, not gated)."""
import os

import numpy as np
import pytest

from tests import sim3_solver_model as M
from tests import sim3_solver_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_header_declares_what_the_model_assumes():
    header = open(os.path.join(ROOT, "include", "orbfe.h")).read()
    assert "#define ORBFE_SIM3_RANSAC_LDS_SLOTS %d" % S.LDS_SLOTS in header
    for name in ("orbfe_enqueue_sim3_ransac_batch", "orbfe_enqueue_sim3_ransac_select", "orbfe_sim3_ransac"):
        assert name + "(" in header
    from orbslam2_amd import api
    import ctypes as C
    assert C.sizeof(api.Sim3RansacCandidate) == 64 and api.SIM3_HYP_DTYPE == M.HYP_DTYPE and api.SIM3_RANSAC_LDS_SLOTS == S.LDS_SLOTS


def test_known_similarity_is_recovered_from_three_exact_points():
    """90 degrees about z, scale 2, a translation."""
    P2 = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1.5]], f32).T.copy()
    Rz = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float64)
    t = np.array([0.5, -1.0, 2.0])
    P1 = (2 * Rz @ P2.astype(np.float64) + t[:, None]).astype(f32)
    R, tt, s, sR, sRinv, tinv = M.compute_sim3(P1, P2, False)
    assert np.abs(R - Rz).max() < 1e-6 and np.abs(tt - t).max() < 1e-6 and abs(float(s) - 2.0) < 1e-6
    assert np.abs(sR - 2 * Rz).max() < 1e-6 and np.abs(sRinv @ sR - np.eye(3)).max() < 1e-6 and np.abs(sRinv @ tt + tinv).max() < 1e-6
    _, _, s1, _, _, _ = M.compute_sim3(P1, P2, True)
    assert s1.dtype == f32 and s1.tobytes() == f32(1.0).tobytes()       # fix_scale: exactly 1.0f


def test_jacobi_diagonalises_and_the_top_vector_is_not_mixed():
    """Three points: M has rank 2 and N's spectrum is +-(s1 + s2), +-(s1 - s2); the two-sided Jacobi separates +lambda from -lambda."""
    rng = np.random.default_rng(5)
    for _ in range(50):
        P1, P2 = rng.normal(size=(3, 3)).astype(f32), rng.normal(size=(3, 3)).astype(f32)
        N = M.horn_n(M._matmul(M.centroid(P2)[0], M.centroid(P1)[0].T))
        d, V, sweeps = M.jacobi4(N)
        V = np.array(V)
        assert sweeps < 12
        assert np.abs(V.T @ N.astype(np.float64) @ V - np.diag(d)).max() < 1e-12 * max(1.0, np.abs(N).max())
        w = np.linalg.eigvalsh(N.astype(np.float64))
        assert np.allclose(sorted(d), w, atol=1e-12 * max(1.0, np.abs(N).max()))
        assert abs(w[0] + w[3]) < 1e-5 * w[3]                          # the spectrum really is symmetric: the trap of a one-sided Jacobi


def test_event_rule_on_hand_written_counts():
    assert M.events_of([5, 21, 21, 20, 25, 25, 30, 29], 20) == [1, 2, 4, 5, 6]    # ties with the record return again
    assert M.events_of([20, 20, 20], 20) == []                                    # a count equal to min_inliers never returns
    assert M.events_of([30, 21, 29, 30], 20) == [0, 3]                            # below the record: no return, even above the floor
    assert M.events_of([0, 0, 21], 20) == [2]
    assert M.events_of([], 20) == []


def test_random_int_and_the_draws():
    assert M.random_int(0, 40) == 0 and M.random_int(M.RAND_MAX, 40) == 39 and M.random_int(M.RAND_MAX, 1) == 0
    N = 10
    raw = lambda i, d: int(np.ceil(i * 2147483648.0 / d))             # the smallest raw value that RandomInt maps to i
    assert M.draw_set([raw(4, 10), raw(4, 9), raw(4, 8)], N) == (4, 9, 8)         # the second draw lands on the vacated position: the old back
    assert M.draw_set([raw(9, 10), raw(8, 9), raw(7, 8)], N) == (9, 8, 7)         # always the back itself
    assert M.draw_set([raw(8, 10), raw(8, 9), raw(8 - 1, 8)], N) == (8, 9, 7)
    assert M.draw_set([0, 0, 0], N) == (0, 9, 8)
    rng = np.random.default_rng(1)
    for _ in range(2000):                                             # against the literal array form
        N = int(rng.integers(3, 30))
        r = rng.integers(0, M.RAND_MAX + 1, 3)
        avail, ids = list(range(N)), []
        for i in range(3):
            k = M.random_int(r[i], len(avail))
            ids.append(avail[k]); avail[k] = avail[-1]; avail.pop()
        assert M.draw_set(r, N) == tuple(ids)


def test_iteration_table():
    t = M.its_table(400, 0.99, 20, 300)
    assert (t[:20] == 0).all() and t[20] == 1 and t[40] == 35 and t[400] == 300 and t[21] == 3
    assert M.its_table(40, 0.99, 9, 300)[40] == 300                   # what the 300-hypothesis scenes rely on
    assert M.iterations_for(10 ** 6, 0.99, 20, 300) == 300            # log(1 - eps^3) rounds to -0: clamped before the conversion


def test_truncated_gate_makes_an_outlier():
    """mvnMaxError1 is a vector<size_t>: 9.21 * sigma2 is truncated to 9 on level 0.  The scene asserts that its error lies in [9, 9.21)."""
    K, J, e1, e2, g1, g2 = S.gate_case()
    print("truncated gate: hypothesis %d correspondence %d err1 %.4f (gate %.0f) err2 %.4f (gate %.0f)" % (K, J, e1, g1, e2, g2))
    m = S.model("gate")
    assert g1 == 9.0 and 9.0 <= e1 < 9.21 and e2 < g2
    assert not (m["bits"][K][J >> 5] >> np.uint32(J & 31)) & 1
    assert m["hyp"]["n_inliers"][K] == m["n_corr"] - 1
    assert M.gate(S.SIGMA2[0]) == 9.0 and M.gate(S.SIGMA2[1]) == 13.0 and float(f32(9.21) * S.SIGMA2[1]) > 13.2


def test_coincident_triple():
    m = S.model("coincident")
    assert tuple(m["sets"][0]) == (0, 1, 2)
    h = m["hyp"][0]
    assert h["n_inliers"] == 0 and not m["bits"][0].any()
    assert np.array_equal(h["R12"], np.eye(3, dtype=f32).reshape(9))                 # the zero vector part: R = I, not 0 / 0
    assert h["s12"].view(np.uint32) == M.NAN_BITS and (h["t12"].view(np.uint32) == M.NAN_BITS).all()
    rest = m["hyp"][1:m["n_its"]]
    assert np.isfinite(rest["s12"]).all() and np.isfinite(rest["R12"]).all() and np.isfinite(rest["t12"]).all()
    assert rest["n_inliers"].max() > 30


def test_filter_keeps_pair_order_and_skips_invalid_slots():
    s, m = S.scene("invalid_slots"), S.model("invalid_slots")
    assert m["n_corr"] == 37 and m["status"] == 0                      # pairs 3, 7 and 20 lose a side
    keep = [k for k in range(40) if k not in (3, 7, 20)]
    assert np.array_equal(m["corr"][:37], s["pairs"][keep]) and (m["corr"][37:] == -1).all()
    assert S.model("below_min")["n_its"] == 0 and S.model("below_min")["n_events"] == 0
    assert S.model("at_min")["n_its"] == 1


@pytest.mark.parametrize("name", S.RANDOM_SCENES)
def test_classifications_equal_the_float64_path(name):
    cases, left, bad, dev = S.near_gate_census(name)
    print("%s: %d cases, %d within 1e-3 of a gate, %d disagreements outside them, max |R, t, s - float64 path| %.3e" % (name, cases, left, bad, dev))
    assert cases == 12000
    assert bad == 0
    assert left <= cases // 1000


def test_iterate_replay_equals_the_literal_transcription():
    """The event walk (what ORB_SLAM2::Sim3Solver::iterate does, here in Python) against the literal loop, on the scenes' counts and on
    hand-written ones whose event falls on the last iteration."""
    rows = [(S.model(n)["n_corr"], S.model(n)["hyp"]["n_inliers"][:S.model(n)["n_its"]], S.scene(n)["min_inliers"]) for n in ("outliers", "clean", "n65", "at_min", "below_min")]
    rows += [(40, np.array(c, np.int32), 20) for c in LAST_ITERATION_COUNTS]
    for N, counts, mn in rows:
        for step in (1, 5, 300):
            assert event_walk(N, counts, mn, step) == literal_walk(N, counts, mn, step)
    log = literal_walk(40, np.array(LAST_ITERATION_COUNTS[0], np.int32), 20, 5)
    assert log[-2][:2] == (9, False) and log[-1][:2] == (-1, True)     # the return on the last iteration leaves bNoMore false until the next call


LAST_ITERATION_COUNTS = [[3, 20, 7, 19, 0, 20, 1, 2, 3, 25], [30, 30, 2, 31], [21], [0, 0, 0, 0, 0], [22, 21, 5, 22, 22, 4, 3, 2, 1, 0, 23]]


def literal_walk(N, counts, min_inliers, step):
    s = M.Solver(N, counts, min_inliers, max(1, len(counts)))
    log = []
    while True:
        k, no_more, n = s.iterate(step)
        log.append((k, no_more, n, s.mnIterations if N >= min_inliers else 0))
        if no_more:
            return log
        assert len(log) < 4096


def event_walk(N, counts, min_inliers, step):
    ev, max_its = M.events_of(counts, min_inliers), max(1, len(counts))
    it, log = 0, []
    while True:
        if N < min_inliers:
            log.append((-1, True, 0, 0))
            return log
        end = min(max_its, it + step)
        nxt = [e for e in ev if it <= e < end]
        if nxt:
            it = nxt[0] + 1
            log.append((nxt[0], False, int(counts[nxt[0]]), it))
        else:
            it = max(it, end)
            log.append((-1, it >= max_its, 0, it))
            if it >= max_its:
                return log
        assert len(log) < 4096
