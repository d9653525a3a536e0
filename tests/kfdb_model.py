"""A plain model of the keyframe database's queries, written from the reference text, with a trace of the branches taken.

score()  fbow::fBow::score                                  Thirdparty/fbow/src/fbow.cpp:206-256
loop()   KeyFrameDatabase::DetectLoopCandidates             src/KeyFrameDatabase.cc:73-194
reloc()  KeyFrameDatabase::DetectRelocalizationCandidates   src/KeyFrameDatabase.cc:196-307

A database is a list of (words, weights, dead): words ascending uint32, weights float32.  An erased keyframe (dead) is in no
inverted-file list (KeyFrameDatabase::erase, :46-62), a live keyframe without words is in none either, so both contribute
nothing; the indices of both stay.  covis[k] = keyframe k's GetBestCovisibilityKeyFrames list, LONGER than 10 where a scene
wants to show that only the first 10 count (the reference cuts it in the call, :149 / :263).  An erased keyframe listed as a
neighbour is skipped: the reference's covisibility graph forgets a bad keyframe (KeyFrame::SetBadFlag), the entry points keep
the index and look at nothing of it.

What is and is not observable.  score() multiplies in float32 (the map's value type is a float, fbow.cpp:223 `vi * wi`), adds
in float64 in word order and takes the square root in float64; the result is rounded to float32 (the callers' `float si`,
KeyFrameDatabase.cc:130 / :247).  The ORDER of the additions is not observable at float32 output.  Measured when
this model was written, on random cases of 100-5000 query words with unit-norm weights spanning nine decades, a keyframe sharing
a third to all of them: the float32 score under sequential, reversed, pairwise-tree and per-64-chunk summation differed in 0 of
200 cases and in 0 of 2000 more (the issue that asked for this model reports 0 of 200 on cases of its own).  What does show on
the same cases: the product taken in float64, 9 of 200 and 148 of 2000 (29 of 200 there), and a float32 square root, 191 of 200
and 1905 of 2000 (1303 of 2000 there).  So no test built on this model claims to pin the association order, MUTANTS holds no
summation-order mutant, and nothing is asserted about one.

MUTANTS are deliberate errors, one per name, that tests/test_kfdb_model.py must tell from the true model on the scenes of
tests/kfdb_scenes.py: each is a way a kernel or a selection could be subtly wrong.
"""
import numpy as np

F32 = np.float32

MUTANTS = (
    "prod_double",        # product not rounded to float32
    "sqrtf",              # square root in float32
    "signed_cmp",         # word ids compared as int32
    "drop_lane63",        # the keyframe's words at positions 63 mod 64 are not looked up
    "first_kf_word",      # first-encounter key = the keyframe's first word, not its first SHARED word
    "first_chunk0",       # first-encounter key only taken from the keyframe's first 64 words
    "min_common_ge",      # >= for > at minCommonWords
    "retain_ge",          # >= for > at minScoreToRetain
    "min_score_gt",       # > for >= at minScore
    "covis_11",           # 11 covisibility entries read
    "fresh_state",        # a filtered neighbour contributes this query's score, not its stale mRelocScore
    "connected_in_max",   # connected keyframes counted into maxCommonWords
    "index_order",        # keyframes sharing words walked in index order, not first-encounter order
    "no_dedupe",          # spAlreadyAddedKF ignored
)

KERNEL_MUTANTS = ("signed_cmp", "drop_lane63", "first_kf_word", "first_chunk0")

# branch counters of the selections; REQUIRED = each must be seen in the union over the scenes
REQUIRED = [
    "no_sharing",
    "max_common_1", "max_common_4", "max_common_5", "max_common_6", "max_common_16",
    "common_eq_min_dropped", "common_eq_min_plus1_kept",
    "covis_len_0", "covis_len_10", "covis_len_11_tail_matters",
    "neigh_self", "neigh_twice", "neigh_erased", "neigh_no_word", "neigh_filtered_stale_nonzero", "neigh_passing",
    "best_moves", "neigh_equal_score_not_taken",
    "acc_eq_retain_dropped", "dedupe",
    "order_differs_from_index", "same_first_word_index_order",
    "loop_connected_would_raise_max", "loop_neigh_connected_skipped", "loop_below_min_score_feeds",
    "loop_score_eq_min_kept", "loop_all_connected", "loop_connected_null",
]
RECORDED = ["queries", "candidates", "scored", "retain_dropped", "neigh_filtered", "loop_below_min_score"]


def new_trace():
    return {k: 0 for k in REQUIRED + RECORDED}


def _lt(a, b, mutant):
    if mutant == "signed_cmp":
        return (a - (1 << 32) if a >> 31 else a) < (b - (1 << 32) if b >> 31 else b)
    return a < b


def score(q, kf, mutant=None):
    """fBow::score(q, kf) as the callers keep it (float32), the number of shared words and the first shared word (None: none).
    fbow.cpp:216-245 is a merge-join of two maps ordered by word id; :223 adds the float product to a double."""
    (w1, v1), (w2, v2) = q, kf
    w1, w2 = np.asarray(w1, np.uint32).tolist(), np.asarray(w2, np.uint32).tolist()   # plain ints: the walk below is per word
    n1, n2 = len(w1), len(w2)
    a = b = 0
    s = 0.0                                       # double score = 0 (:214)
    common, first = 0, None
    while a < n1 and b < n2:                      # :216
        if mutant == "drop_lane63" and b % 64 == 63:
            b += 1
            continue
        if w1[a] == w2[b]:                        # :221
            if mutant == "prod_double":
                s += float(v1[a]) * float(v2[b])
            else:
                s += float(F32(v1[a]) * F32(v2[b]))   # :223 float * float, then += into the double
            if first is None:
                first = w1[a]
                if mutant == "first_kf_word":
                    first = w2[0]
                if mutant == "first_chunk0" and b >= 64:
                    first = 0xFFFFFFFF
            common += 1
            a += 1; b += 1
        elif _lt(w1[a], w2[b], mutant):           # :229-235
            while a < n1 and _lt(w1[a], w2[b], mutant):
                a += 1
        else:                                     # :236-244
            while b < n2 and _lt(w2[b], w1[a], mutant):
                b += 1
    if s >= 1:                                    # :250
        sc = 1.0
    elif mutant == "sqrtf":
        sc = 1.0 - float(np.sqrt(F32(1.0 - s)))
    else:
        sc = 1.0 - float(np.sqrt(np.float64(1.0 - s)))   # :253
    return F32(sc), common, first


def scores(db, q, mutant=None):
    """(common int32[n], score float32[n], first[n]) of every keyframe: what orbfe_kfdb_score answers (erased: 0 / 0.0)."""
    n = len(db)
    common = np.zeros(n, np.int32); sc = np.zeros(n, np.float32); first = [None] * n
    for k, (w, v, dead) in enumerate(db):
        if dead or len(w) == 0 or len(q[0]) == 0:
            continue
        sc[k], common[k], first[k] = score(q, (w, v), mutant)
    return common, sc, first


def _sharing(db, q, skip, mutant, tr):
    """:82-102 / :204-220.  The inverted file lists a word's keyframes in the order they were added; the query's words are
    walked in ascending order.  Returns the list in first-encounter order and the shared-word counts."""
    common, sc, first = scores(db, q, mutant)
    if mutant in KERNEL_MUTANTS:                  # a wrong kernel: what the selection would make of its (common, first)
        ks = [k for k in range(len(db)) if common[k] > 0 and not skip[k]]
        ks.sort(key=lambda k: (first[k], k))
    else:                                         # the reference's walk, literally
        inv = {}
        for k, (w, v, dead) in enumerate(db):
            if not dead:
                for x in np.asarray(w, np.uint32).tolist():
                    inv.setdefault(x, []).append(k)               # KeyFrameDatabase::add :38-44
        ks, words = [], {}
        for x in np.asarray(q[0], np.uint32).tolist():            # :83 / :204
            for k in inv.get(x, ()):                              # :87 / :208
                if skip[k]:
                    continue                                      # :94 (a connected keyframe's count is never read)
                if k not in words:
                    words[k] = 0
                    ks.append(k)
                words[k] += 1
        assert all(words[k] == common[k] for k in ks) and len(ks) == sum(1 for k in range(len(db)) if common[k] > 0 and not skip[k])
        if mutant == "index_order":
            ks.sort()
    if ks != sorted(ks):
        tr["order_differs_from_index"] += 1
    if any(first[a] == first[b] for a, b in zip(ks, ks[1:])):
        tr["same_first_word_index_order"] += 1
    return ks, common, sc


def _min_common(max_common, tr):
    key = "max_common_%d" % max_common
    if key in tr:
        tr[key] += 1
    return int(F32(max_common) * F32(0.8))        # int minCommonWords = maxCommonWords*0.8f (:118 / :233): float product


def _accumulate(k, own, covis, counted, value, tr, mutant, db):
    """:146-171 / :260-285 for one keyframe: (accScore, pBestKF).  counted(k2) = the neighbour's test, value(k2) its score."""
    def walk(nn, count):
        best, acc, bk = own, own, k
        seen = set()
        for k2 in covis[k][:nn]:
            if count:
                tr["neigh_self"] += k2 == k
                tr["neigh_twice"] += k2 in seen
                seen.add(k2)
            if not counted(k2, count):
                continue
            v = value(k2)
            acc = F32(acc + v)                    # float accScore
            if v > best:
                if count:
                    tr["best_moves"] += 1
                bk, best = k2, v
            elif count and v == best and k2 != bk:
                tr["neigh_equal_score_not_taken"] += 1
        return acc, bk
    n = len(covis[k])
    tr["covis_len_0"] += n == 0
    tr["covis_len_10"] += n == 10
    acc, bk = walk(10, True)                      # GetBestCovisibilityKeyFrames(10)
    if n > 10 and walk(n, False) != (acc, bk):
        tr["covis_len_11_tail_matters"] += 1
    if mutant == "covis_11":
        acc, bk = walk(11, False)
    return acc, bk


def _retain(order, acc, best_kf, best_acc, tr, mutant):
    """:173-191 / :287-304"""
    min_retain = F32(0.75) * F32(best_acc)
    out = []
    for i in range(len(order)):
        if acc[i] > min_retain or (mutant == "retain_ge" and acc[i] == min_retain):
            if best_kf[i] in out and mutant != "no_dedupe":
                tr["dedupe"] += 1
            else:
                out.append(best_kf[i])
        else:
            tr["retain_dropped"] += 1
            tr["acc_eq_retain_dropped"] += acc[i] == min_retain
    tr["candidates"] += len(out)
    return out


def reloc(db, q, covis, state, mutant=None):
    """DetectRelocalizationCandidates.  state = every keyframe's mRelocScore before the query (float32, not modified).
    Returns (candidates, state after, trace)."""
    tr = new_trace(); tr["queries"] = 1
    state = np.array(state, np.float32)
    n = len(db)
    ks, common, sc = _sharing(db, q, [False] * n, mutant, tr)
    if not ks:                                    # :222
        tr["no_sharing"] += 1
        return [], state, tr
    min_common = _min_common(max(int(common[k]) for k in ks), tr)   # :226-233
    sm = []
    for k in ks:                                  # :240-251
        if common[k] > min_common or (mutant == "min_common_ge" and common[k] == min_common):
            tr["common_eq_min_plus1_kept"] += common[k] == min_common + 1
            state[k] = sc[k]
            sm.append(k)
        else:
            tr["common_eq_min_dropped"] += common[k] == min_common
    tr["scored"] += len(sm)
    if not sm:
        return [], state, tr

    def counted(k2, count):                       # :271 mnRelocQuery != F->mnId
        dead = db[k2][2]
        if count:
            tr["neigh_erased"] += bool(dead)
            tr["neigh_no_word"] += (not dead) and common[k2] == 0
        if dead or common[k2] == 0:
            return False
        if count:
            if k2 in sm:
                tr["neigh_passing"] += 1
            else:
                tr["neigh_filtered"] += 1
                tr["neigh_filtered_stale_nonzero"] += state[k2] != 0
        return True

    def value(k2):                                # :274 pKF2->mRelocScore, whenever it was written
        return sc[k2] if mutant == "fresh_state" else state[k2]

    acc, best_kf, best_acc = [], [], F32(0)       # :257
    for k in sm:
        a, bk = _accumulate(k, sc[k], covis, counted, value, tr, mutant, db)
        acc.append(a); best_kf.append(bk)
        if a > best_acc:
            best_acc = a
    return _retain(sm, acc, best_kf, best_acc, tr, mutant), state, tr


def loop(db, q, connected, min_score, covis, mutant=None):
    """DetectLoopCandidates(pKF, minScore).  connected = flag per keyframe (pKF->GetConnectedKeyFrames()) or None.
    Stateless: returns (candidates, None, trace)."""
    tr = new_trace(); tr["queries"] = 1
    n = len(db)
    min_score = F32(min_score)
    tr["loop_connected_null"] += connected is None
    conn = [False] * n if connected is None else [bool(c) for c in connected]
    ks, common, sc = _sharing(db, q, conn, mutant, tr)        # :94 connected keyframes never enter the list
    if not ks:                                    # :105
        if any(common[k] > 0 for k in range(n)):
            tr["loop_all_connected"] += 1
        else:
            tr["no_sharing"] += 1
        return [], None, tr
    max_common = max(int(common[k]) for k in ks)  # :111-116, over the list only
    if any(conn[k] and common[k] > max_common for k in range(n)):
        tr["loop_connected_would_raise_max"] += 1
        if mutant == "connected_in_max":
            max_common = max(int(common[k]) for k in range(n))
    min_common = _min_common(max_common, tr)
    scored, sm = set(), []
    for k in ks:                                  # :122-136
        if common[k] > min_common or (mutant == "min_common_ge" and common[k] == min_common):
            tr["common_eq_min_plus1_kept"] += common[k] == min_common + 1
            scored.add(k)                         # mLoopScore = si
            if sc[k] > min_score or (mutant != "min_score_gt" and sc[k] == min_score):
                tr["loop_score_eq_min_kept"] += sc[k] == min_score
                sm.append(k)
            else:
                tr["loop_below_min_score"] += 1
        else:
            tr["common_eq_min_dropped"] += common[k] == min_common
    tr["scored"] += len(scored)
    if not sm:                                    # :138
        return [], None, tr

    def counted(k2, count):                       # :157 mnLoopQuery == pKF->mnId && mnLoopWords > minCommonWords
        dead = db[k2][2]
        if count:
            tr["neigh_erased"] += bool(dead)
            tr["neigh_no_word"] += (not dead) and common[k2] == 0
            tr["loop_neigh_connected_skipped"] += conn[k2] and common[k2] > 0
        if k2 not in scored:
            if count and not dead and common[k2] > 0 and not conn[k2]:
                tr["neigh_filtered"] += 1
            return False
        if count:
            tr["neigh_passing"] += 1
            tr["loop_below_min_score_feeds"] += k2 not in sm
        return True

    acc, best_kf, best_acc = [], [], min_score    # :142
    for k in sm:
        a, bk = _accumulate(k, sc[k], covis, counted, lambda k2: sc[k2], tr, mutant, db)
        acc.append(a); best_kf.append(bk)
        if a > best_acc:
            best_acc = a
    return _retain(sm, acc, best_kf, best_acc, tr, mutant), None, tr
