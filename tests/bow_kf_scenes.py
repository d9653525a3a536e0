"""Scenes, oracle binding, variants and census for ORBmatcher::SearchByFboW(KeyFrame*, KeyFrame*) (src/ORBmatcher.cc:517-650) on
device-resident keyframes (tests/test_bow_kf_device.py).  No test here; everything is computed once, cached and never changed.

A keyframe is a dict: fv = (nodes, off, feat) CSR, valid (int32), d (n x 32 bytes), ang (float32).  A scene is (kf1, kf2).

big_node()     hand-made feature vectors, no vocabulary: KF2 nodes of up to 4200 features, so that winners lie beyond the 128 list
               positions a lane keeps in registers and beyond the 4096 its flag register covers; KF1 features whose best candidate is
               already taken (vbMatched2), has no good map point (valid2), lies at exactly TH_LOW, or is tied with a second one.
single_node()  one shared node, one descriptor on each side, 4 bits apart: every step is a tie of all free KF2 keypoints.
family()       one KF1 of 1500 keypoints (the keyframe of tests/test_bow_device.py) against six candidates, vocabulary feature
               vectors, for the batch; small_candidates() 70 more.
census()       a plain restatement of the reference's loop (vectorised over a node's KF2 list) that counts the event classes and,
               per `variant`, breaks one rule on purpose: what a wrong kernel would compute.
"""
import ctypes as C

import numpy as np

from oracle import oracle as O
from tests import test_bow as TB
from tests import test_bow_device as TD
from tests import test_bow_device_batch as TDB
from tests import triangulation_scenes as TS

TH_LOW, HISTO_LENGTH = 50, 30
SETTINGS = ((0.75, True), (0.9, False), (1.25, True))  # (nnratio, check_ori); the last one accepts ties
BIG_LAYOUT = {3: (40, 70), 7: (10, 0), 8: (90, 150), 9: (0, 25), 20: (48, 4200), 41: (66, 30), 50: (0, 12)}  # node id -> (n1, n2)
NODE_SIZES = (1, 63, 64, 65, 128, 129)
FAMILY = ["perturbed", "sparse", "tiny", "self", "novalid", "big"]
VARIANTS = ("ignore_matched2", "ignore_valid2", "le_th_low", "best2_skips_duplicates")
_p = TB._p
_CACHE = {}


def _kf(fv, valid, d, ang):
    ang = np.ascontiguousarray(ang, np.float32)
    ang[ang >= 360] = 0  # a double just below 360 may round up to it
    return dict(fv=tuple(np.ascontiguousarray(a, t) for a, t in zip(fv, (np.uint32, np.int32, np.int32))),
                valid=np.ascontiguousarray(valid, np.int32), d=np.ascontiguousarray(d, np.uint8), ang=ang)


# ------------------------------------------------------------------ oracle
def oracle(kf1, kf2, ratio, ori, valid1=None):
    """orc_search_by_bow_kf (oracle/orb_oracle_bow.c): (match12, count)."""
    L = O.lib()
    L.orc_search_by_bow_kf.restype = C.c_int
    L.orc_search_by_bow_kf.argtypes = ([C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 3 + [C.c_int]) * 2 + [C.c_float, C.c_int, C.c_void_p]
    v1 = kf1["valid"] if valid1 is None else np.ascontiguousarray(valid1, np.int32)
    n1 = len(kf1["d"])
    ref = np.zeros(max(n1, 1), np.int32)
    a, b = kf1["fv"], kf2["fv"]
    nref = L.orc_search_by_bow_kf(_p(a[0]), _p(a[1]), _p(a[2]), len(a[0]), _p(v1), _p(kf1["d"]), _p(kf1["ang"]), n1,
                                  _p(b[0]), _p(b[1]), _p(b[2]), len(b[0]), _p(kf2["valid"]), _p(kf2["d"]), _p(kf2["ang"]), len(kf2["d"]),
                                  ratio, int(ori), _p(ref))
    return ref[:n1].copy(), nref


def literal(kf1, kf2, ratio, ori):
    """oracle/literal_bow.py: search_by_fbow_kf_kf, the line-by-line transcription."""
    from oracle import literal_bow as LB

    def as_map(fv):
        return {int(nid): [int(i) for i in fv[2][fv[1][k]:fv[1][k + 1]]] for k, nid in enumerate(fv[0])}

    return LB.search_by_fbow_kf_kf(as_map(kf1["fv"]), kf1["valid"], kf1["d"], kf1["ang"], len(kf1["d"]),
                                   as_map(kf2["fv"]), kf2["valid"], kf2["d"], kf2["ang"], ratio, ori)


pairs_of = TS.pairs_of


# ------------------------------------------------------------------ big nodes
def big_node(seed=91):
    key = ("big", seed)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(seed)
    ids = sorted(BIG_LAYOUT)
    n1 = sum(BIG_LAYOUT[i][0] for i in ids); n2 = sum(BIG_LAYOUT[i][1] for i in ids)
    assert (n1, n2) == (254, 4487) and n1 % 64 and n2 % 64

    def csr(side, n):
        perm = rng.permutation(n)
        nodes, off, feat, p = [], [0], [], 0
        for i in ids:
            c = BIG_LAYOUT[i][side]
            if c == 0:
                continue
            nodes.append(i); feat += sorted(perm[p:p + c].tolist()); p += c; off.append(p)
        return np.array(nodes, np.uint32), np.array(off, np.int32), np.array(feat, np.int32)

    fv1, fv2 = csr(0, n1), csr(1, n2)
    # both sides start as filler: descriptors ~128 bits from everything, random angles
    d1 = rng.integers(0, 256, (n1, 32)).astype(np.uint8); d2 = rng.integers(0, 256, (n2, 32)).astype(np.uint8)
    a1 = rng.uniform(0, 359.9, n1); a2 = rng.uniform(0, 359.9, n2)
    v1 = (rng.random(n1) < 0.9).astype(np.int32); v2 = (rng.random(n2) < 0.85).astype(np.int32)
    node2_at = {int(nid): b for b, nid in enumerate(fv2[0])}

    def twin(idx1, idx2, bits, valid=1, random_angle=False):
        d2[idx2] = TS._flip(rng, d1[idx1], bits)
        v2[idx2] = valid
        a2[idx2] = rng.uniform(0, 359.9) if random_angle else (a1[idx1] + rng.normal(0, 4)) % 360

    far_done = 0
    for a, nid in enumerate(fv1[0]):
        b = node2_at.get(int(nid))
        if b is None:
            continue
        seg1 = fv1[2][fv1[1][a]:fv1[1][a + 1]]
        seg2 = fv2[2][fv2[1][b]:fv2[1][b + 1]]
        pool = rng.permutation(len(seg2)).tolist()           # free list positions of the KF2 node
        far = [p for p in pool if p >= 4096]                 # ... and those beyond the 64 flag bits of a lane
        pool = [p for p in pool if p < 4096]
        for i, idx1 in enumerate(seg1):
            if i % 4 == 3:                                   # duplicates its predecessor: meets the flag its predecessor left
                d1[idx1] = d1[seg1[i - 1]]; a1[idx1] = a1[seg1[i - 1]]; v1[idx1] = 1
                continue
            kind = rng.choice(["plain", "invalid_best", "at_th_low", "tie"], p=[0.55, 0.15, 0.15, 0.15])
            if int(nid) == 20 and i % 4 == 2 and far_done < 10 and len(far) >= 2:
                # two twins beyond list position 4096: this feature takes the closer one, its duplicate (i + 1) must find that flag in
                # memory and take the other
                v1[idx1] = 1
                twin(idx1, seg2[far.pop()], 0); twin(idx1, seg2[far.pop()], 5)
                far_done += 1
                continue
            if i % 4 == 2:
                v1[idx1] = 1                                 # so that its duplicate's flag matters
            if kind == "plain":
                for _ in range(int(rng.integers(1, 4))):
                    if pool:
                        twin(idx1, seg2[pool.pop()], int(rng.choice([0, 3, 8, 11, 30, 49])), random_angle=rng.random() < 0.2)
            elif kind == "invalid_best" and len(pool) >= 2:  # the closest candidate has no good map point
                twin(idx1, seg2[pool.pop()], 2, valid=0); twin(idx1, seg2[pool.pop()], 9)
            elif kind == "at_th_low" and pool:               # bestDist1 == TH_LOW: `<` rejects, `<=` would accept
                twin(idx1, seg2[pool.pop()], TH_LOW); v1[idx1] = 1
            elif kind == "tie" and len(pool) >= 2:           # two candidates at the best distance: bestDist2 == bestDist1
                j, k = seg2[pool.pop()], seg2[pool.pop()]
                twin(idx1, j, 6); d2[k] = d2[j]; v2[k] = 1; a2[k] = a2[j]; v1[idx1] = 1
    assert far_done >= 8
    out = (_kf(fv1, v1, d1, a1), _kf(fv2, v2, d2, a2))
    _CACHE[key] = out
    return out


def single_node(n1, n2, seed=5):
    """One shared node; every KF2 descriptor is the same and 4 bits from every KF1 descriptor.  With nnratio <= 1 a KF1 feature is
    accepted only while a single KF2 keypoint is free; above 1 the first free one in list order wins every step."""
    key = ("single", n1, n2, seed)
    if key not in _CACHE:
        rng = np.random.default_rng(seed)
        desc = rng.integers(0, 256, 32).astype(np.uint8)

        def kf(n, d):
            fv = (np.array([5], np.uint32), np.array([0, n], np.int32), np.arange(n, dtype=np.int32))
            return _kf(fv, np.ones(n, np.int32), np.tile(d, (n, 1)), np.full(n, 10.0, np.float32))

        _CACHE[key] = (kf(n1, desc), kf(n2, TS._flip(rng, desc, 4)))
    return _CACHE[key]


def scenes():
    """name -> (kf1, kf2): what the CPU tests compare oracle and literal on and the GPU test runs through the single call."""
    out = {"big_node": big_node()}
    for n2 in NODE_SIZES:
        out["single_node_%d" % n2] = single_node(5, n2)
    return out


# ------------------------------------------------------------------ the candidate family (vocabulary feature vectors)
def _transform(d):
    if "voc" not in _CACHE:
        _CACHE["voc"] = TB._oracle_voc(TD._vocab())
    L, v = _CACHE["voc"]
    return TB._oracle_transform(L, v, d, 4)[2]


def _cand(kf1, seed, n_copy, n_noise, flip, pvalid, dang):
    c = TDB._cand(kf1["d"], kf1["ang"], seed, n_copy, n_noise, flip, pvalid, dang)
    return _kf(_transform(c["d"]), c["valid"], c["d"], c["ang"])


def kf1_of_family():
    if "kf1" not in _CACHE:
        sc = TD._scene()
        _CACHE["kf1"] = _kf(_transform(sc["kf_d"]), sc["kf_valid"], sc["kf_d"], sc["kf_ang"])
    return _CACHE["kf1"]


def _big_candidate(kf1, seed=17):
    """300 perturbed copies of KF1 keypoints in their nodes, then 4200 filler keypoints in KF1's most populous node, then twins of
    that node's KF1 keypoints: these lie beyond position 4096 of the node's list."""
    rng = np.random.default_rng(seed)
    nodes1, off1, feat1 = kf1["fv"]
    node_of = np.zeros(len(kf1["d"]), np.int64)
    for k in range(len(nodes1)):
        node_of[feat1[off1[k]:off1[k + 1]]] = nodes1[k]
    top = int(np.argmax(np.diff(off1)))
    members = feat1[off1[top]:off1[top + 1]]
    src = rng.permutation(len(kf1["d"]))[:300]
    d = np.concatenate([TB._descs(seed + 1, 0, base=kf1["d"][src], flip=0.03), rng.integers(0, 256, (4200, 32)).astype(np.uint8),
                        TB._descs(seed + 2, 0, base=kf1["d"][members], flip=0.01)])
    ang = np.concatenate([(kf1["ang"][src] + rng.normal(0, 5, 300)) % 360, rng.uniform(0, 359.9, 4200), (kf1["ang"][members] + rng.normal(0, 3, len(members))) % 360])
    node = np.concatenate([node_of[src], np.full(4200 + len(members), nodes1[top])])
    order = np.argsort(node, kind="stable")                 # inside a node the features ascend
    ids, counts = np.unique(node, return_counts=True)
    valid = (rng.random(len(d)) < 0.9).astype(np.int32)
    valid[-len(members):] = 1
    return _kf((ids, np.concatenate([[0], np.cumsum(counts)]), order), valid, d, ang)


def family():
    """(kf1, [candidates in FAMILY order]); KF1 has 1500 keypoints."""
    if "family" not in _CACHE:
        kf1 = kf1_of_family()
        perturbed = _cand(kf1, 11, 1300, 400, 0.03, 0.9, 5)
        fam = dict(perturbed=perturbed, sparse=_cand(kf1, 12, 500, 300, 0.06, 0.5, 40), tiny=_cand(kf1, 13, 40, 0, 0.03, 1.0, 3),
                   self=kf1, novalid=dict(perturbed, valid=np.zeros_like(perturbed["valid"])), big=_big_candidate(kf1))
        _CACHE["family"] = (kf1, [fam[name] for name in FAMILY])
    return _CACHE["family"]


def small_candidates(count=70):
    if ("small", count) not in _CACHE:
        kf1 = kf1_of_family()
        _CACHE[("small", count)] = [_cand(kf1, 300 + k, 150, 50, 0.03, 0.85, 5) for k in range(count)]
    return _CACHE[("small", count)]


# ------------------------------------------------------------------ census
def census(kf1, kf2, ratio, ori, variant=None):
    """The loop of :537-616 and the rotation cut of :619-633 with the inner loop as arrays over a node's KF2 list.  Returns
    (match12, count, classes).  `variant` (one of VARIANTS) breaks one rule; classes are only meaningful without one."""
    assert variant is None or variant in VARIANTS
    f32 = np.float32
    n1, n2 = len(kf1["d"]), len(kf2["d"])
    bits1, bits2 = np.unpackbits(kf1["d"], axis=1), np.unpackbits(kf2["d"], axis=1)
    match12 = np.full(n1, -1, np.int32)
    matched2 = np.zeros(n2, bool)
    cls = dict(pos64=0, pos128=0, pos4096=0, second_round=0, flag_changed=0, valid2_changed=0, at_th_low=0, tie_rejected=0, pruned=0,
               only_kf1=0, only_kf2=0)
    hist = [[] for _ in range(HISTO_LENGTH)]
    at2 = {int(nid): j for j, nid in enumerate(kf2["fv"][0])}
    cls["only_kf2"] = len(set(at2) - set(int(x) for x in kf1["fv"][0]))

    def best(mask, d):
        """(position of the first minimum or -1, bestDist1, bestDist2) of the if-chain of :577-587 over the candidates in mask."""
        ok = np.nonzero(mask)[0]
        if len(ok) == 0:
            return -1, 256, 256
        w = int(ok[np.argmin(d[ok])])  # argmin: the first of the equals
        rest = ok[ok != w]
        if variant == "best2_skips_duplicates":
            rest = rest[d[rest] != d[w]]
        return w, int(d[w]), int(d[rest].min()) if len(rest) else 256

    def accepted(b1, b2):
        return (b1 <= TH_LOW if variant == "le_th_low" else b1 < TH_LOW) and f32(b1) < f32(ratio) * f32(b2)

    for i, nid in enumerate(kf1["fv"][0]):
        j = at2.get(int(nid))
        if j is None:
            cls["only_kf1"] += 1
            continue
        seg1 = kf1["fv"][2][kf1["fv"][1][i]:kf1["fv"][1][i + 1]]
        seg2 = kf2["fv"][2][kf2["fv"][1][j]:kf2["fv"][1][j + 1]]
        cls["second_round"] += int(kf1["valid"][seg1].sum() > 64)
        good2 = kf2["valid"][seg2] != 0
        for idx1 in seg1:
            if not kf1["valid"][idx1]:
                continue
            d = (bits1[idx1][None, :] ^ bits2[seg2]).sum(axis=1)
            free = ~matched2[seg2]
            mask = (good2 if variant != "ignore_valid2" else np.ones(len(seg2), bool)) & (free if variant != "ignore_matched2" else True)
            w, b1, b2 = best(mask, d)
            ok = w >= 0 and accepted(b1, b2)
            if variant is None:
                for name, other in (("flag_changed", good2), ("valid2_changed", free)):
                    w_o, b1_o, b2_o = best(other, d)
                    ok_o = w_o >= 0 and accepted(b1_o, b2_o)
                    cls[name] += (ok_o != ok) or (ok and w_o != w)
                cls["at_th_low"] += int(w >= 0 and b1 == TH_LOW and f32(b1) < f32(ratio) * f32(b2))
                cls["tie_rejected"] += int(w >= 0 and b1 < TH_LOW and b2 == b1 and not ok)
            if not ok:
                continue
            cls["pos64"] += w >= 64; cls["pos128"] += w >= 128; cls["pos4096"] += w >= 4096
            match12[idx1] = seg2[w]; matched2[seg2[w]] = True
            if ori:
                hist[TS._rot_bin(kf1["ang"][idx1], kf2["ang"][seg2[w]])].append(idx1)
    if ori:
        keep = TS._three_maxima([len(h) for h in hist])
        for bin_, h in enumerate(hist):
            if bin_ not in keep:
                match12[h] = -1
                cls["pruned"] += len(h)
    return match12, int((match12 >= 0).sum()), {k: int(v) for k, v in cls.items()}
