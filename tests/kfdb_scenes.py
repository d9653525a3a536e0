"""Scenes for the census of the keyframe database (tests/test_kfdb_model.py on the CPU, tests/test_gpu_kfdb_census.py on the GPU).

A scene is one small database and a sequence of queries on it, so that mRelocScore carries over between the queries:

    name      str
    db        [(words uint32 ascending, weights float32, dead bool)]   at most 64 keyframes of at most ~300 words
    covis     [[keyframe index]] per keyframe, in GetBestCovisibilityKeyFrames order, possibly longer than 10
    queries   [{"q": (words, weights), "loops": [(connected flags or None, min_score)]}]
    oracle    False where the oracle cannot hold the scene (it sizes an inverted file by the largest word id); such scenes are
              compared with the model only, on the CPU there is nothing else to compare them with

No vocabulary: every vector is hand-made or seeded.  The selection scenes use a query of 16 words of weight 0.25, for which a
keyframe sharing m of them at weight 0.25 scores exactly 1 - sqrt(1 - m / 16): 1.0 (m = 16), 0.75 (15), 0.5 (12), 0.25 (7).
"""
import os
import re

import numpy as np

from tests import kfdb_model as M

HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "orbslam2_amd", "csrc", "orbfe_bow.hip")

NQ_SMALL = (1, 63, 64, 65)
KF_LENGTHS = (0, 1, 63, 64, 65, 128, 129, 200)
PATTERNS = ("none", "first", "last", "lane63", "chunk1", "full_chunk", "chunks_0_2", "all")
LONG = 5000


def kfdb_q_lds():
    """KFDB_Q_LDS as orbfe_bow.hip defines it: the longest query the score kernel stages in LDS."""
    with open(HIP) as f:
        m = re.search(r"^#define\s+KFDB_Q_LDS\s+(\d+)", f.read(), re.M)
    assert m, "KFDB_Q_LDS is no longer defined in orbfe_bow.hip"
    return int(m.group(1))


def _u(a):
    return np.array(a, np.uint32)


def _f(a):
    return np.array(a, np.float32)


def _unit(rng, n):
    v = rng.uniform(0.05, 1.0, n)
    return (v / np.sqrt((v * v).sum())).astype(np.float32) if n else np.zeros(0, np.float32)


def _scene(name, db, queries, covis=None, oracle=True):
    db = [(_u(w), _f(v), bool(d)) for w, v, d in db]
    for w, v, d in db:
        assert len(w) == len(v) and (np.diff(w.astype(np.int64)) > 0).all()
    qs = []
    for q in queries:
        w, v = _u(q["q"][0]), _f(q["q"][1])
        assert len(w) == len(v) and (np.diff(w.astype(np.int64)) > 0).all()
        qs.append({"q": (w, v), "loops": list(q.get("loops", [(None, 0.0)]))})
    return {"name": name, "db": db, "covis": covis if covis is not None else [[] for _ in db], "queries": qs, "oracle": oracle}


# ---------------------------------------------------------------- the kernel's grid

def pattern_positions(pat, n):
    """Positions of a keyframe of n words that the query hits, or None where the pattern needs a longer keyframe."""
    if pat == "none":
        return []
    if n == 0:
        return None
    if pat == "first":
        return [0]
    if pat == "last":
        return [n - 1]
    if pat == "all":
        return list(range(n))
    if pat == "lane63":                         # only the last lane of the first 64-word chunk
        return [63] if n >= 64 else None
    if pat == "chunk1":                         # the first shared word lies in the second chunk
        return list(range(64, min(n, 128), 3)) if n >= 65 else None
    if pat == "full_chunk":                     # all 64 lanes of chunk 0 hit, nothing else
        return list(range(64)) if n >= 64 else None
    if pat == "chunks_0_2":                     # hits in chunks 0 and 2, none in chunk 1
        return [5, 128] + ([150] if n > 150 else []) if n >= 129 else None
    raise KeyError(pat)


STRIDE = 64     # keyframe k's word at position j is STRIDE * (j + 1) + k + 1: no two keyframes share a word, and multiples of STRIDE belong to nobody


def _grid_db(rng):
    db = []
    for rep in range(3):
        for n in KF_LENGTHS:
            k = len(db)
            db.append((STRIDE * (np.arange(n) + 1) + k + 1, _unit(rng, n), False))
    return db


def _grid_query(db, nq, shift, rng):
    """A query of exactly nq words: the patterns, rotated by `shift` (and by 3 more per repetition of the lengths, so that
    shifts 0, 1, 2 give every length every pattern), dealt to the keyframes while their hits fit, then words
    nobody has: word id 0 and further ones below every keyframe word, the rest above every keyframe word."""
    words = []
    for k, (w, v, dead) in enumerate(db):
        pos = pattern_positions(PATTERNS[(k + 3 * (k // len(KF_LENGTHS)) + shift) % len(PATTERNS)], len(w))
        if pos is None or len(words) + len(pos) > nq:
            pos = []
        words += [int(w[j]) for j in pos]
    top = STRIDE * 400
    fill = [0, 7, 13][: min(3, nq - len(words))]
    fill += [top + STRIDE * t for t in range(nq - len(words) - len(fill))]
    words = np.array(sorted(words + fill), np.uint32)
    assert len(words) == nq and len(np.unique(words)) == nq
    return (words, _unit(rng, nq))


def grid_scenes():
    q_lds = kfdb_q_lds()
    out = []
    rng = np.random.default_rng(20)
    db = _grid_db(rng)
    qs = []
    for i, nq in enumerate(NQ_SMALL + (8, 200, 300)):
        for shift in (0, 1, 2):
            qs.append({"q": _grid_query(db, nq, shift, rng)})
    out.append(_scene("grid_short_queries", db, qs))
    for i, nq in enumerate((q_lds - 1, q_lds, q_lds + 1, LONG)):
        rng = np.random.default_rng(30 + i)
        db = _grid_db(rng)
        out.append(_scene("grid_nq_%s" % ("lds_minus_1", "lds", "lds_plus_1", "long")[i], db,
                          [{"q": _grid_query(db, nq, s, rng)} for s in (0, 1, 2)]))
    return out


def weight_scenes():
    q64 = (np.arange(64) * 3 + 5, np.full(64, 0.125))                 # 64 x 2^-6 = 1 exactly
    q256 = (np.arange(256) * 2 + 1, np.full(256, 0.0625))
    rng = np.random.default_rng(41)
    over = None
    for seed in range(200):                                           # a unit vector whose float32 squares sum past 1
        v = _unit(np.random.default_rng(1000 + seed), 40)
        if sum(float(np.float32(x) * np.float32(x)) for x in v) > 1.0:
            over = (np.arange(40) * 5 + 2, v)
            break
    assert over is not None
    tiny = (np.array([9, 11, 400]), np.full(3, 2.0 ** -30))           # products 2^-60: their sum is below 2^-53
    db = [(q64[0], q64[1], False), (q256[0], q256[1], False), (over[0], over[1], False), (tiny[0], tiny[1], False),
          (np.arange(90) * 7 + 3, _unit(rng, 90), False)]
    return [_scene("weights", db, [{"q": q64}, {"q": q256}, {"q": over}, {"q": tiny}, {"q": (db[4][0][::2], _unit(rng, 45))}])]


def huge_id_scenes():
    """Word ids 0 and 0x7fffffff, the largest fbow can produce (bit 31 is its leaf flag), and ids with bit 31 set, which the
    uint32 interface accepts: only with those does a signed comparison of word ids show.  The oracle would size its inverted
    file by the largest id, so these scenes are compared with the model only."""
    top = 0x7FFFFFFF
    rng = np.random.default_rng(43)
    db = [([0, 5, top], _unit(rng, 3), False), ([0], [1.0], False), ([top], [1.0], False), ([1, top - 1], [0.6, 0.8], False),
          ([3, top - 2, top], _unit(rng, 3), True)]
    a = _scene("word_ids_0_and_max", db, [{"q": ([0, top], [0.6, 0.8])}, {"q": ([0], [1.0])}, {"q": ([top], [1.0])},
                                           {"q": ([2, 4, top - 1], _unit(rng, 3))}], oracle=False)
    hi = 0x80000001
    db = [([5, 9, hi, 0xFFFFFFFE], _unit(rng, 4), False), ([hi, hi + 7], [0.6, 0.8], False), ([5, 0xFFFFFFFE], [0.8, 0.6], False)]
    b = _scene("word_ids_with_bit_31", db, [{"q": ([5, hi, 0xFFFFFFFE], _unit(rng, 3))}, {"q": ([9, hi + 7], [0.6, 0.8])}], oracle=False)
    return [a, b]


def live_count_scenes():
    """1..9 live keyframes (the last workgroup of four waves is partly idle unless the count is a multiple of 4) between erased
    ones at index 0, in the middle and last; one live keyframe without words among them from 3 on."""
    out = []
    for n_live in range(1, 10):
        rng = np.random.default_rng(50 + n_live)
        vocab = np.arange(1, 120)
        kfs = []
        for k in range(n_live):
            n = 0 if (k == 1 and n_live >= 3) else int(rng.integers(1, 80))
            kfs.append((np.sort(rng.choice(vocab, n, replace=False)), _unit(rng, n), False))
        dead = lambda: (np.sort(rng.choice(vocab, 30, replace=False)), _unit(rng, 30), True)
        mid = (n_live + 1) // 2
        db = [dead()] + kfs[:mid] + [dead(), dead()] + kfs[mid:] + [dead()]
        n = len(db)
        covis = [[int(x) for x in rng.integers(0, n, int(rng.integers(0, 5)))] for _ in range(n)]
        qs = []
        for j in range(2):
            nq = int(rng.integers(20, 70))
            conn = (rng.random(n) < 0.2).astype(np.uint8)
            qs.append({"q": (np.sort(rng.choice(vocab, nq, replace=False)), _unit(rng, nq)), "loops": [(conn, 0.05), (None, 0.0)]})
        out.append(_scene("live_%d" % n_live, db, qs, covis))
    return out


# ---------------------------------------------------------------- the selections' branches

Q16 = np.arange(16) * 10 + 100            # the 16-word query, weight 0.25 each


def _q16():
    return (Q16, np.full(16, 0.25))


def _share(keep, foreign_base):
    """A 16-word keyframe of weight 0.25: the query's words at the positions in `keep`, foreign words for the rest."""
    keep = sorted(keep)
    w = [int(Q16[i]) for i in keep] + [foreign_base + 1 + 2 * i for i in range(16 - len(keep))]
    return (np.array(sorted(w)), np.full(16, 0.25), False)


def selection_scenes():
    out = []
    R = range
    # --- the retain cut: acc == 0.75f * best_acc exactly is dropped; common == min_common dropped, min_common + 1 kept
    db = [_share(R(16), 1000), _share(R(15), 1100), _share(R(12), 1200), _share(R(13), 1300)]
    out.append(_scene("retain_tie", db, [{"q": _q16(), "loops": [(None, 0.0), (None, 0.75), (None, float(np.nextafter(np.float32(0.75), np.float32(1)))),
                                                             ([1, 1, 1, 1], 0.0)]}]))
    # --- max_common 1, 4, 5, 6: float32 min_common 0, 3, 4, 4
    for mc in (1, 4, 5, 6):
        mn = int(np.float32(mc) * np.float32(0.8))
        qw = np.arange(mc) * 10 + 100
        db = []
        for c in (mn, mc, mn + 1, 1, 0):                      # shares c words, weights unit norm over max(c, 1) + 1 words
            w = sorted([int(x) for x in qw[mc - c:]] + [2000 + 10 * len(db)])
            db.append((w, np.full(len(w), 1.0 / np.sqrt(len(w))), False))
        out.append(_scene("max_common_%d" % mc, db, [{"q": (qw, np.full(mc, 1.0 / np.sqrt(mc))), "loops": [(None, 0.0), (None, 0.3)]}]))
    # --- nothing shared, empty and erased databases are the GPU file's degenerate cases; here: a live database, foreign query
    out.append(_scene("no_sharing", [_share(R(16), 1000), ([], [], False)], [{"q": ([1, 2, 3], [0.6, 0.0, 0.8])}]))
    # --- covisibility: every kind of neighbour
    db = [
        _share(R(16), 1000),                   # 0: 1.0
        _share(R(1, 16), 1100),                # 1: 0.75, first shared word 110
        _share(R(15), 1200),                   # 2: 0.75
        _share(R(13), 1300),                   # 3: 13 words
        _share(R(12), 1400),                   # 4: 12 == min_common: filtered in the second query, scored in the first
        _share(R(14), 1500),                   # 5: erased
        ([1, 2, 3], [0.6, 0.0, 0.8], False),   # 6: shares nothing
        _share(R(14), 1700),                   # 7: 14 words
        ([], [], False),                       # 8: live, no words
        _share(R(2, 16), 1900),                # 9: 14 words, first shared word 120
        _share(R(3, 16), 2000),                # 10: 13 words
    ]
    db[5] = (db[5][0], db[5][1], True)
    covis = [[] for _ in db]
    covis[1] = [1, 2, 2, 5, 6, 4, 3]                     # itself, an equal score (not taken), twice, erased, no word, filtered (stale), passing
    covis[2] = [0]                                       # best moves to 0, which is also its own group's best: one entry
    covis[3] = [6, 8, 6, 8, 6, 8, 6, 8, 6, 10]           # exactly 10
    covis[9] = [10, 6, 6, 6, 6, 6, 6, 6, 6, 6, 0]        # 11: the last would take `best` and raise `acc`
    covis[10] = [4]
    q_first = (Q16[:12], np.full(12, 0.25))              # keyframe 4 shares all 12: scored, its mRelocScore is written
    conn = np.zeros(len(db), np.uint8); conn[0] = 1
    out.append(_scene("covisibility", db, [{"q": q_first}, {"q": _q16(), "loops": [(None, 0.0), (conn, 0.0), (conn, 0.75), (None, 0.6)]},
                                           {"q": (Q16[4:], np.full(12, 0.25))}], covis))
    # --- the eleventh entry, visibly: read, it would make keyframe 1 the best of keyframe 0's group
    db = [_share(R(15), 1000), _share(R(16), 1100), _share(R(13), 1200), ([1, 2], [0.6, 0.8], False)]
    covis = [[2] + [3] * 9 + [1], [], [], []]
    out.append(_scene("eleventh_entry", db, [{"q": _q16()}], covis))
    # --- first-encounter order: chunk 1, a small first word that is not shared, equal first words
    qw = np.array([1000, 2000, 3000, 4000, 5000]); qv = np.full(5, 1.0 / np.sqrt(5.0))
    low = list(range(1, 71))

    def kf(lows, shared, extra):
        w = sorted(lows + shared + extra)
        v = np.full(len(w), 0.01); v[[w.index(x) for x in shared]] = 0.5
        return (w, v, False)
    db = [kf(low, [3000, 4000, 5000], []), kf([], [2000, 3000, 4000], [9000]), kf(low, [1000, 2000, 3000], []),
          kf([], [2000, 4000, 5000], [9001]), kf([5], [2000, 3000, 5000], [])]
    out.append(_scene("first_encounter_order", db, [{"q": (qw, qv)}]))
    # --- loop only: connected keyframes leave max_common, a connected neighbour is unscored, minScore
    db = [
        _share(R(16), 1000),                   # 0: connected; would raise max_common from 13 to 16
        _share(R(13), 1100),                   # 1: 13 words
        _share(R(11), 1200),                   # 2: 11 > int(13 * 0.8f) = 10, but not > int(16 * 0.8f) = 12
        _share(R(10), 1300),                   # 3: 10 == min_common
        _share(R(3, 16), 1400),                # 4: 13 words
    ]
    covis = [[], [0, 2], [1], [], [2, 0]]
    conn = [1, 0, 0, 0, 0]
    s13 = float(M.score(_q16(), db[1][:2])[0]); s11 = float(M.score(_q16(), db[2][:2])[0])
    below = float(np.nextafter(np.float32(s11), np.float32(1)))              # keyframe 2 is just below it and still feeds 1 and 4
    out.append(_scene("loop_connected", db, [{"q": _q16(), "loops": [(conn, 0.0), (conn, s11), (conn, below), (conn, s13), (None, 0.0),
                                                                    ([1] * 5, 0.0), ([1, 1, 0, 0, 1], 0.0)]}], covis))
    return out


_SCENES = []


def scenes():
    """Every scene, built once; callers must not modify them."""
    if not _SCENES:
        _SCENES.extend(selection_scenes() + weight_scenes() + huge_id_scenes() + live_count_scenes() + grid_scenes())
    return _SCENES


# ---------------------------------------------------------------- the model's answers and the census

_RUNS = {}


def run_model(scene, mutant=None):
    """Per query: {"common", "score", "reloc": candidates, "state": mRelocScore after, "loops": [candidates], "traces": [...]}.
    The true model's answers are computed once and shared."""
    key = (scene["name"], mutant)
    if mutant is None and key in _RUNS:
        return _RUNS[key]
    state = np.zeros(len(scene["db"]), np.float32)
    res = []
    for q in scene["queries"]:
        common, sc, _ = M.scores(scene["db"], q["q"], mutant)
        cand, state, tr = M.reloc(scene["db"], q["q"], scene["covis"], state, mutant)
        r = {"common": common, "score": sc, "reloc": cand, "state": state.copy(), "loops": [], "traces": [tr]}
        for conn, ms in q["loops"]:
            c, _, tr = M.loop(scene["db"], q["q"], conn, ms, scene["covis"], mutant)
            r["loops"].append(c); r["traces"].append(tr)
        res.append(r)
    if mutant is None:
        _RUNS[key] = res
    return res


def same(a, b):
    return all(np.array_equal(x["common"], y["common"]) and np.array_equal(x["score"].view(np.uint32), y["score"].view(np.uint32)) and
               x["reloc"] == y["reloc"] and np.array_equal(x["state"].view(np.uint32), y["state"].view(np.uint32)) and x["loops"] == y["loops"]
               for x, y in zip(a, b))


KERNEL_REQUIRED = ["score_exactly_1_identical", "sum_above_1", "common_but_score_0", "live_keyframe_without_words", "erased_keyframe",
                   "first_hit_in_chunk_1", "only_lane_63", "only_lane_0", "all_64_lanes", "chunks_0_and_2_not_1", "no_hit",
                   "query_below_all_keyframe_words", "query_above_all_keyframe_words"]


def kernel_census(scene):
    """What the score kernel meets in a scene, counted from the scene's data alone."""
    c = {k: 0 for k in KERNEL_REQUIRED}
    res = run_model(scene)
    for q, r in zip(scene["queries"], res):
        qw = q["q"][0]
        for k, (w, v, dead) in enumerate(scene["db"]):
            c["erased_keyframe"] += dead
            c["live_keyframe_without_words"] += (not dead) and len(w) == 0
            if dead or len(w) == 0:
                continue
            pos = np.nonzero(np.isin(w, qw))[0]
            chunks = set((pos // 64).tolist())
            c["no_hit"] += len(pos) == 0
            c["first_hit_in_chunk_1"] += len(pos) > 0 and pos[0] // 64 == 1
            c["only_lane_63"] += pos.tolist() == [63]
            c["only_lane_0"] += pos.tolist() == [0] and len(w) >= 64
            c["all_64_lanes"] += len(pos) == 64 and chunks == {0}
            c["chunks_0_and_2_not_1"] += chunks == {0, 2}
            c["query_below_all_keyframe_words"] += qw.max() < w.min()
            c["query_above_all_keyframe_words"] += qw.min() > w.max()
            same_vec = len(w) == len(qw) and np.array_equal(w, qw) and np.array_equal(v, q["q"][1])
            s = sum(float(np.float32(a) * np.float32(b)) for a, b in zip(v[pos], q["q"][1][np.isin(qw, w)]))
            c["score_exactly_1_identical"] += same_vec and r["score"][k] == 1.0
            c["sum_above_1"] += s > 1.0
            c["common_but_score_0"] += len(pos) > 0 and r["score"][k] == 0.0
    return {k: int(v) for k, v in c.items()}


def census():
    """Per scene and in union: the selections' branch counters (kfdb_model.REQUIRED + RECORDED) and the kernel's (KERNEL_REQUIRED)."""
    out = {"scenes": {}, "union": {k: 0 for k in M.REQUIRED + M.RECORDED + KERNEL_REQUIRED}}
    for s in scenes():
        c = {k: 0 for k in M.REQUIRED + M.RECORDED}
        for r in run_model(s):
            for tr in r["traces"]:
                for k, v in tr.items():
                    c[k] += int(v)
        c.update(kernel_census(s))
        out["scenes"][s["name"]] = c
        for k, v in c.items():
            out["union"][k] += v
    return out
