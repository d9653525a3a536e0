"""The keyframe database's census on the CPU: the plain model of tests/kfdb_model.py equals the oracle bit for bit on every scene
of tests/kfdb_scenes.py that the oracle can hold, the union of the model's traces (kept in tests/golden/kfdb_census.json) shows
every required branch of the two selections and every edge of the score kernel's grid, the query lengths straddle the kernel's
LDS / HBM switch as orbfe_bow.hip defines it today, and every deliberate error of kfdb_model.MUTANTS changes the answer of at
least one scene -- so the GPU comparison of tests/test_gpu_kfdb_census.py, which is against the same answers, would see a kernel
or a selection with that error.

Not claimed: the order of the additions in fBow::score.  It cannot be seen in the float32 result (kfdb_model's docstring has
the measurement), so there is no summation-order mutant and nothing is asserted about one.

Only the model can check the scenes `word_ids_0_and_max` and `word_ids_with_bit_31` (the oracle sizes an inverted file by the
largest word id): no REQUIRED branch depends on them, of the mutants only `signed_cmp` does."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import kfdb_model as M
from tests import kfdb_scenes as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kfdb_census.json")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _oracle():
    from oracle import oracle as O
    L = O.lib()
    L.orc_bow_score.restype = C.c_double
    L.orc_bow_score.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    L.orc_detect_reloc_candidates.restype = C.c_int
    L.orc_detect_reloc_candidates.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_int]
    L.orc_detect_loop_candidates.restype = C.c_int
    L.orc_detect_loop_candidates.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_float] + [C.c_void_p] * 3 + [C.c_int]
    return L


def _csr(lists, dtype):
    off = np.zeros(len(lists) + 1, np.int32); off[1:] = np.cumsum([len(x) for x in lists])
    flat = np.concatenate([np.asarray(x, dtype) for x in lists] + [np.zeros(1, dtype)])   # never empty
    return off, np.ascontiguousarray(flat)


def test_model_equals_oracle_bit_for_bit():
    L = _oracle()
    n_scenes = 0
    for s in S.scenes():
        if not s["oracle"]:
            continue
        n_scenes += 1
        n = len(s["db"])
        live = [(w, v) if not dead else (w[:0], v[:0]) for w, v, dead in s["db"]]        # the oracle's erased keyframe: no words
        kf_off, dbw = _csr([w for w, _ in live], np.uint32)
        _, dbv = _csr([v for _, v in live], np.float32)
        c_off, c_idx = _csr(s["covis"], np.int32)          # whole lists: the oracle reads 10 of them too
        state = np.zeros(n, np.float32)
        cand = np.zeros(n, np.int32)
        for qi, (q, r) in enumerate(zip(s["queries"], S.run_model(s))):
            qw, qv = q["q"]
            for k, (w, v) in enumerate(live):
                if len(w):
                    ref = np.float32(L.orc_bow_score(_p(qw), _p(qv), len(qw), _p(w), _p(v), len(w)))
                    assert ref.view(np.uint32) == r["score"][k].view(np.uint32), (s["name"], qi, k, ref, r["score"][k])
                    assert r["common"][k] == len(np.intersect1d(qw, w)), (s["name"], qi, k)
                else:
                    assert r["common"][k] == 0 and r["score"][k] == 0, (s["name"], qi, k)
            m = L.orc_detect_reloc_candidates(_p(qw), _p(qv), len(qw), n, _p(kf_off), _p(dbw), _p(dbv), _p(c_off), _p(c_idx), _p(state), _p(cand), n)
            assert cand[:m].tolist() == r["reloc"], (s["name"], qi)
            assert np.array_equal(state.view(np.uint32), r["state"].view(np.uint32)), (s["name"], qi)
            for (conn, ms), want in zip(q["loops"], r["loops"]):
                cn = None if conn is None else np.ascontiguousarray(conn, np.uint8)
                m = L.orc_detect_loop_candidates(_p(qw), _p(qv), len(qw), n, _p(kf_off), _p(dbw), _p(dbv), None if cn is None else _p(cn), float(ms),
                                                 _p(c_off), _p(c_idx), _p(cand), n)
                assert cand[:m].tolist() == want, (s["name"], qi, ms)
    assert n_scenes == len(S.scenes()) - 2


def test_issue_known_answer_of_the_retain_tie():
    """16 words of weight 0.25; A identical (1.0), B shares 15 (0.9375 -> exactly 0.75): acc == 0.75f * best_acc is dropped."""
    s = next(s for s in S.scenes() if s["name"] == "retain_tie")
    r = S.run_model(s)[0]
    assert r["reloc"] == [0] and r["state"][:2].tolist() == [1.0, 0.75]
    assert [int(np.float32(x) * np.float32(0.8)) for x in (1, 4, 5, 6, 16)] == [0, 3, 4, 4, 12]


def test_census_shows_every_required_branch():
    got = S.census()
    with open(GOLDEN) as f:
        want = json.load(f)
    assert got == want, "tests/golden/kfdb_census.json no longer matches the model's traces (regenerate it with kfdb_scenes.census())"
    for item in M.REQUIRED + S.KERNEL_REQUIRED:
        assert want["union"][item] >= 1, item
    assert set(want["union"]) == set(M.REQUIRED + M.RECORDED + S.KERNEL_REQUIRED)
    assert set(want["scenes"]) == {s["name"] for s in S.scenes()}


def test_scenes_span_the_kernels_grid_and_its_lds_boundary():
    """If KFDB_Q_LDS moves, the scenes move with it (they read it) and this still sees both sides of the branch."""
    q = S.kfdb_q_lds()
    nqs = {len(x["q"][0]) for s in S.scenes() for x in s["queries"]}
    assert {1, 63, 64, 65, q - 1, q, q + 1, S.LONG} <= nqs and S.LONG > q + 1000
    for s in S.scenes():
        assert len(s["db"]) <= 64 and all(len(w) <= 300 for w, _, _ in s["db"]), s["name"]
        assert len(s["covis"]) == len(s["db"]) and all(0 <= k2 < len(s["db"]) for c in s["covis"] for k2 in c), s["name"]
    # every keyframe length met by every hit pattern it admits, on both sides of the boundary
    for side in (lambda n: n <= q, lambda n: n > q):
        met = set()
        for s in S.scenes():
            if not s["name"].startswith("grid_"):
                continue
            for x in s["queries"]:
                if not side(len(x["q"][0])):
                    continue
                for w, _, dead in s["db"]:
                    pos = np.nonzero(np.isin(w, x["q"][0]))[0].tolist()
                    for pat in S.PATTERNS:
                        if S.pattern_positions(pat, len(w)) == pos:
                            met.add((len(w), pat))
        want = {(n, pat) for n in S.KF_LENGTHS for pat in S.PATTERNS if S.pattern_positions(pat, n) is not None}
        assert want <= met, sorted(want - met)
    live = {sum(1 for _, _, d in s["db"] if not d) for s in S.scenes() if s["name"].startswith("live_")}
    assert live == set(range(1, 10))
    for s in S.scenes():
        if s["name"].startswith("live_"):
            dead = [d for _, _, d in s["db"]]
            assert dead[0] and dead[-1] and any(dead[1:-1]), s["name"]
    ids = {int(x) for s in S.scenes() for w, _, _ in s["db"] for x in w} & {int(x) for s in S.scenes() for q_ in s["queries"] for x in q_["q"][0]}
    assert {0, 0x7FFFFFFF} <= ids


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_every_wrong_kernel_or_selection_is_seen(mutant):
    seen = [s["name"] for s in S.scenes() if not S.same(S.run_model(s), S.run_model(s, mutant))]
    assert seen, "no scene tells the mutant %r from the model: the scenes are missing a case" % mutant


def test_shared_answers_are_computed_once_and_leave_the_scenes_alone():
    """The shared answers stay as computed: run_model returns the same objects, and the scenes' arrays are unchanged by it."""
    s = S.scenes()[0]
    before = [(w.copy(), v.copy()) for w, v, _ in s["db"]]
    a = S.run_model(s); b = S.run_model(s)
    assert a is b
    assert all(np.array_equal(w, w0) and np.array_equal(v, v0) for (w, v, _), (w0, v0) in zip(s["db"], before))
