"""The keyframe database's census on the GPU: kfdb_score_kernel and the two host selections of orbfe_bow.hip against the plain
model of tests/kfdb_model.py on every scene of tests/kfdb_scenes.py -- for EVERY keyframe of every query the shared-word count
and the float32 bits of the score, the candidate lists in order, and mRelocScore after every query of a scene's sequence.  The
scenes reach both query paths of the kernel (LDS up to KFDB_Q_LDS words, HBM beyond), the chunk and wave edges of a keyframe,
live counts 1..9 between erased keyframes, and every selection branch tests/golden/kfdb_census.json lists;
tests/test_kfdb_model.py shows on the CPU that a kernel or selection with any of kfdb_model.MUTANTS' errors would differ from
these answers.  All comparisons are exact; the order of fBow::score's additions is not claimed (kfdb_model's docstring).

Then the same scenes on an aged database (growths of the word arrays, erased keyframes before and after the scene's, a
compaction that moves the scene's live segments), a regrowing scratch buffer, and the raw C interface: ORBFE_ERR_CAPACITY, NULL
outputs of orbfe_kfdb_score, guard cells, degenerate inputs, and queries that are not strictly ascending (refused)."""
import ctypes as C

import numpy as np
import pytest

from tests import kfdb_model as M
from tests import kfdb_scenes as S

pytestmark = pytest.mark.gpu

PREFIX = 20          # aged database: keyframes added (and later erased) before the scene's, and as many after
PREFIX_WORDS = 300


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def ctx():
    from orbslam2_amd import api
    c = api.Context(width=640, height=480, nfeatures=500, max_images=1)
    yield c
    c.close()


def _csr(lists):
    off = np.zeros(len(lists) + 1, np.int32); off[1:] = np.cumsum([len(x) for x in lists])
    return off, np.ascontiguousarray(np.concatenate([np.asarray(x, np.int32) for x in lists] + [np.zeros(1, np.int32)]))


def _load(ctx, scene):
    from orbslam2_amd import bow as B
    db = B.KeyFrameDB(ctx)
    for k, (w, v, dead) in enumerate(scene["db"]):
        assert db.add(w, v) == k
    for k, (w, v, dead) in enumerate(scene["db"]):
        if dead:
            db.erase(k)
    return db


def _check_queries(db, scene, what=""):
    """Every query of the scene, in order, on a loaded database: scores of every keyframe, both selections, the state."""
    want = S.run_model(scene)
    n = len(scene["db"])
    assert len(db) == n
    c_off, c_idx = _csr(scene["covis"])
    state = np.zeros(n, np.float32)
    for qi, (q, r) in enumerate(zip(scene["queries"], want)):
        qw, qv = q["q"]
        at = (what, scene["name"], qi, len(qw))
        common, score = db.score(qw, qv)
        assert np.array_equal(common, r["common"]), (at, np.nonzero(common != r["common"])[0][:8])
        bad = np.nonzero(score.view(np.uint32) != r["score"].view(np.uint32))[0]
        assert len(bad) == 0, (at, bad[:8], score[bad[:8]], r["score"][bad[:8]])
        got = db.detect_reloc_candidates(qw, qv, c_off, c_idx, state)
        assert got.tolist() == r["reloc"], at
        assert np.array_equal(state.view(np.uint32), r["state"].view(np.uint32)), at
        for (conn, ms), cand in zip(q["loops"], r["loops"]):
            got = db.detect_loop_candidates(qw, qv, conn, ms, c_off, c_idx)
            assert got.tolist() == cand, (at, ms)


@pytest.mark.parametrize("name", [s["name"] for s in S.scenes()])
def test_gpu_scene_equals_the_model(ctx, name):
    scene = next(s for s in S.scenes() if s["name"] == name)
    _check_queries(_load(ctx, scene), scene)


def _aged(scene):
    """The scene as the model sees it on the aged database: PREFIX erased keyframes before its own and PREFIX after."""
    qw, qv = scene["queries"][0]["q"]
    rng = np.random.default_rng(7)
    span = np.unique(np.concatenate([qw[:PREFIX_WORDS], np.arange(1, 2 * PREFIX_WORDS, dtype=np.uint32)]))

    def old():   # would share words with the first query if it were not erased
        w = np.sort(rng.choice(span, PREFIX_WORDS, replace=False)).astype(np.uint32)
        v = rng.uniform(0.1, 1.0, PREFIX_WORDS); v = (v / np.sqrt((v * v).sum())).astype(np.float32)
        return (w, v, True)
    db = [old() for _ in range(PREFIX)] + scene["db"] + [old() for _ in range(PREFIX)]
    covis = [[] for _ in range(PREFIX)] + [[k2 + PREFIX for k2 in c] for c in scene["covis"]] + [[1, PREFIX, len(db) - 1] for _ in range(PREFIX)]
    qs = []
    for q in scene["queries"]:
        loops = [(None if conn is None else np.concatenate([np.zeros(PREFIX, np.uint8), np.asarray(conn, np.uint8), np.ones(PREFIX, np.uint8)]), ms)
                 for conn, ms in q["loops"]]
        qs.append({"q": q["q"], "loops": loops})
    return {"name": scene["name"] + "@aged", "db": db, "covis": covis, "queries": qs, "oracle": False}


def _replay_storage(lengths_and_erases):
    """The word arrays' bookkeeping as orbfe_kfdb_add / _erase document it (grow to 2 * need + 1024 when full; compact when the
    dead words exceed 1024 and half of the used ones): (growths, compactions, growths with live words to move)."""
    cap = used = dead = 0
    growths = compactions = moving = 0
    length, gone = [], []
    for op, x in lengths_and_erases:
        if op == "add":
            if used + x > cap:
                cap = 2 * (used + x) + 1024
                growths += 1
                moving += used > 0
            length.append(x); gone.append(False); used += x
        else:
            dead += length[x]; gone[x] = True
            if dead > 1024 and 2 * dead > used:
                used = sum(n for n, g in zip(length, gone) if not g)
                dead = 0
                compactions += 1
    return growths, compactions, moving


@pytest.mark.parametrize("name", [s["name"] for s in S.scenes()])
def test_gpu_scene_on_an_aged_database(name):
    """A context of its own, so that the word arrays start empty and grow: the keyframes before the scene's force three growths,
    those after it a fourth that moves the scene's words; everything old is erased only once the scene's keyframes are in, which
    compacts the arrays and moves the scene's live segments to the front.  Indices are never reused: the scene's are offset."""
    from orbslam2_amd import api, bow as B
    scene = next(s for s in S.scenes() if s["name"] == name)
    aged = _aged(scene)
    n = len(aged["db"])
    ops = [("add", len(w)) for w, _, _ in aged["db"]] + [("erase", k) for k in range(n) if aged["db"][k][2]]
    growths, compactions, moving = _replay_storage(ops)
    assert growths >= 4 and moving >= 3 and compactions >= 1, (growths, moving, compactions)
    c = api.Context(width=640, height=480, nfeatures=500, max_images=1)
    try:
        db = B.KeyFrameDB(c)
        for k, (w, v, dead) in enumerate(aged["db"]):
            assert db.add(w, v) == k
        q0 = aged["queries"][0]["q"]                        # while everything lives, the old keyframes answer too
        common, score = db.score(*q0)
        wc, ws, _ = M.scores([(w, v, False) for w, v, _ in aged["db"]], q0)
        assert np.array_equal(common, wc) and np.array_equal(score.view(np.uint32), ws.view(np.uint32))
        for k in range(n):
            if aged["db"][k][2]:
                db.erase(k)
        _check_queries(db, aged, "aged")
    finally:
        c.close()


def test_gpu_scratch_regrows_between_short_and_long_queries():
    """short, 5000 words, short again on one fresh context: the query's scratch buffer is reallocated under the database."""
    from orbslam2_amd import api
    scene = next(s for s in S.scenes() if s["name"] == "grid_nq_long")
    long_q = scene["queries"][0]["q"]
    short_q = (long_q[0][::500].copy(), long_q[1][::500].copy())
    c = api.Context(width=640, height=480, nfeatures=500, max_images=1)
    try:
        db = _load(c, scene)
        c_off, c_idx = _csr(scene["covis"])
        state = np.zeros(len(scene["db"]), np.float32); want_state = state.copy()
        for q in (short_q, long_q, short_q, long_q):
            common, score = db.score(*q)
            wc, ws, _ = M.scores(scene["db"], q)
            assert np.array_equal(common, wc) and np.array_equal(score.view(np.uint32), ws.view(np.uint32)), len(q[0])
            cand, want_state, _ = M.reloc(scene["db"], q, scene["covis"], want_state)
            assert db.detect_reloc_candidates(q[0], q[1], c_off, c_idx, state).tolist() == cand
            assert np.array_equal(state.view(np.uint32), want_state.view(np.uint32))
    finally:
        c.close()


# ---------------------------------------------------------------- the raw interface

def _raw(db):
    from orbslam2_amd import api
    L = db.L
    L.orbfe_detect_loop_candidates.restype = C.c_int
    L.orbfe_detect_loop_candidates.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    return L, api


def test_gpu_capacity_error_reports_the_full_count_and_spares_the_guard_cells(ctx):
    scene = next(s for s in S.scenes() if s["name"] == "first_encounter_order")
    db = _load(ctx, scene)
    L, api = _raw(db)
    qw, qv = scene["queries"][0]["q"]
    r = S.run_model(scene)[0]
    want = r["reloc"]
    n = len(want)
    assert n == 5 and r["loops"][0] == want
    c_off, c_idx = _csr(scene["covis"])
    for cap in (n - 1, 0, n):
        for which in ("reloc", "loop"):
            cand = np.full(n + 3, -77, np.int32); got_n = C.c_int(-1)
            state = np.zeros(len(scene["db"]), np.float32)
            ptr = _p(cand) if cap else None
            if which == "reloc":
                rc = L.orbfe_detect_reloc_candidates(ctx.h, _p(qw), _p(qv), len(qw), _p(c_off), _p(c_idx), _p(state), ptr, cap, C.byref(got_n))
                assert np.array_equal(state.view(np.uint32), r["state"].view(np.uint32))     # the state is the query's, whatever fits
            else:
                rc = L.orbfe_detect_loop_candidates(ctx.h, _p(qw), _p(qv), len(qw), None, 0.0, _p(c_off), _p(c_idx), ptr, cap, C.byref(got_n))
            assert rc == (api.OK if cap >= n else api.ERR_CAPACITY), (which, cap, rc)
            assert got_n.value == n, (which, cap)
            assert cand[:cap].tolist() == want[:cap] and (cand[cap:] == -77).all(), (which, cap, cand)


def test_gpu_score_with_null_outputs_and_longer_arrays(ctx):
    scene = next(s for s in S.scenes() if s["name"] == "covisibility")
    db = _load(ctx, scene)
    L, api = _raw(db)
    qw, qv = scene["queries"][1]["q"]
    r = S.run_model(scene)[1]
    n = len(scene["db"])
    common = np.full(n + 5, -77, np.int32); score = np.full(n + 5, -77.0, np.float32)
    assert L.orbfe_kfdb_score(ctx.h, _p(qw), _p(qv), len(qw), _p(common), None) == api.OK
    assert np.array_equal(common[:n], r["common"]) and (common[n:] == -77).all()
    assert L.orbfe_kfdb_score(ctx.h, _p(qw), _p(qv), len(qw), None, _p(score)) == api.OK
    assert np.array_equal(score[:n].view(np.uint32), r["score"].view(np.uint32)) and (score[n:] == -77.0).all()
    assert L.orbfe_kfdb_score(ctx.h, _p(qw), _p(qv), len(qw), None, None) == api.OK
    assert r["common"][5] == 0 and r["score"][5] == 0.0 and scene["db"][5][2]          # the erased keyframe answers 0 / 0.0


def test_gpu_degenerate_queries_and_databases_leave_the_state_alone(ctx):
    from orbslam2_amd import bow as B
    scene = next(s for s in S.scenes() if s["name"] == "covisibility")
    qw, qv = scene["queries"][1]["q"]
    none_w, none_v = np.zeros(0, np.uint32), np.zeros(0, np.float32)
    c_off, c_idx = _csr(scene["covis"])
    n = len(scene["db"])
    marks = (np.arange(n) * 0.125 + 0.5).astype(np.float32)

    def nothing(db, w, v, off=c_off, idx=c_idx):
        state = marks[: max(len(off) - 1, 1)].copy()
        assert db.detect_reloc_candidates(w, v, off, idx, state).tolist() == []
        assert np.array_equal(state, marks[: len(state)])
        assert db.detect_loop_candidates(w, v, None, 0.0, off, idx).tolist() == []
        common, score = db.score(w, v)
        assert len(common) == len(db) and not common.any() and not score.any()

    db = _load(ctx, scene)
    nothing(db, none_w, none_v)                                   # nq == 0
    db = B.KeyFrameDB(ctx)                                        # an empty database
    assert len(db) == 0
    nothing(db, qw, qv, np.zeros(1, np.int32), np.zeros(1, np.int32))
    db = _load(ctx, scene)                                        # every keyframe erased
    for k in range(n):
        db.erase(k)
    nothing(db, qw, qv)
    db = _load(ctx, scene)                                        # and the context still answers
    _check_queries(db, scene, "after the degenerate calls")


@pytest.mark.parametrize("kind", ["repeated", "descending", "repeated_last", "descending_long"])
def test_gpu_query_that_is_not_strictly_ascending_is_refused(ctx, kind):
    """The kernel binary-searches the query; orbfe_kfdb_add refuses the same input for a keyframe."""
    from orbslam2_amd import api
    scene = next(s for s in S.scenes() if s["name"] == "covisibility")
    db = _load(ctx, scene)
    qw, qv = (x.copy() for x in scene["queries"][1]["q"])
    if kind == "repeated":
        qw[3] = qw[2]
    elif kind == "descending":
        qw[[0, 1]] = qw[[1, 0]]
    elif kind == "repeated_last":
        qw[-1] = qw[-2]
    else:                                                         # beyond KFDB_Q_LDS, one swapped pair in the middle
        qw = np.arange(1, S.LONG + 1, dtype=np.uint32) * 3; qv = np.full(S.LONG, 0.01, np.float32)
        qw[[2500, 2501]] = qw[[2501, 2500]]
    c_off, c_idx = _csr(scene["covis"])
    n = len(scene["db"])
    marks = (np.arange(n) * 0.125 + 0.5).astype(np.float32)
    state = marks.copy()
    for call in (lambda: db.score(qw, qv), lambda: db.detect_reloc_candidates(qw, qv, c_off, c_idx, state),
                 lambda: db.detect_loop_candidates(qw, qv, None, 0.0, c_off, c_idx)):
        with pytest.raises(api.OrbfeError) as e:
            call()
        assert e.value.code == api.ERR_INVALID
    assert np.array_equal(state, marks)
    with pytest.raises(api.OrbfeError) as e:                      # as orbfe_kfdb_add does
        db.add(qw, qv)
    assert e.value.code == api.ERR_INVALID and len(db) == n
    _check_queries(db, scene, "after the refusals")
