"""Scenes, oracle binding and census for ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:652-819) on device-resident keyframes
(tests/test_triangulation_device.py).  No test here; everything is computed once and cached.

two_view()   the generator of tests/test_bow.py::test_gpu_search_for_triangulation restated: 1400 points seen from two poses 0.4 m
             apart, feature vectors from the small test vocabulary.  view_of() draws further neighbours of its KF1.
big_node()   hand-made feature vectors, no vocabulary: nodes of up to 4200 KF2 features, so that winners lie beyond the 128 list
             positions a lane keeps in registers and beyond the 4096 its flag register covers, with ties, flags, the epipolar-line
             gate and the epipole disc all changing winners (census()).
census()     a plain restatement of the reference's loop (vectorised over a node's KF2 list) that also counts the event classes.
"""
import ctypes as C

import numpy as np

from oracle import oracle as O
from orbslam2_amd import bow as B
from tests import test_bow as TB

FX = FY = 500.0
CX, CY = 320.0, 240.0
TH_LOW, HISTO_LENGTH = 50, 30
MODES = ((0, 1), (1, 1), (0, 0))  # (only_stereo, check_ori)
BIG_LAYOUT = {3: (40, 70), 7: (10, 0), 8: (90, 150), 9: (0, 25), 20: (100, 4200), 41: (66, 30), 50: (0, 12)}  # node id -> (n1, n2)
_p = TB._p
_CACHE = {}


def levels():
    """mvScaleFactor / mvLevelSigma2 of the default pyramid (8 levels, 1.2), as every context of the tests holds them."""
    if "levels" not in _CACHE:
        ex = O.Extractor()
        _CACHE["levels"] = (np.ascontiguousarray(ex.scale_factors(), np.float32), np.ascontiguousarray(ex.sigma2(), np.float32))
    return _CACHE["levels"]


def _f12(T1, T2):
    """F12 = K^-T [t12]x R12 K^-1 (LocalMapping::ComputeF12), computed in double and handed over as float; Cw1; T2w as float."""
    R12 = T1[:, :3] @ T2[:, :3].T
    t12 = -R12 @ T2[:, 3] + T1[:, 3]
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    K = np.array([[FX, 0, CX], [0, FY, CY], [0, 0, 1.0]])
    F12 = (np.linalg.inv(K).T @ tx @ R12 @ np.linalg.inv(K)).astype(np.float32)
    Cw1 = (-T1[:, :3].T @ T1[:, 3]).astype(np.float32)
    return np.ascontiguousarray(F12), np.ascontiguousarray(Cw1), np.ascontiguousarray(T2.astype(np.float32))


def _yaw(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def _kf(k, d, ur, mp, fv):
    return dict(k=k, d=np.ascontiguousarray(d), ur=np.ascontiguousarray(ur, np.float32), mp=np.ascontiguousarray(mp, np.uint8),
                fv=tuple(np.ascontiguousarray(a, t) for a, t in zip(fv, (np.uint32, np.int32, np.int32))))


# ------------------------------------------------------------------ two-view
def _two_view_base(n):
    if ("tv_base", n) not in _CACHE:
        from orbslam2_amd import api
        if "vocab" not in _CACHE:
            _CACHE["vocab"] = B.build_vocabulary(TB._descs(1, 3000), k=10, levels=5, seed=7)
        vocab = _CACHE["vocab"]
        rng = np.random.default_rng(21)
        P = np.stack([rng.uniform(-6, 6, n), rng.uniform(-4, 4, n), rng.uniform(4, 30, n)], axis=1)
        T1 = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
        T2 = np.concatenate([_yaw(3.0), np.array([[-0.4], [0.02], [0.05]])], axis=1)
        base = (TB._descs(9, n), rng.uniform(0, 360, n))
        L, v = TB._oracle_voc(vocab)

        def view(T, seed):
            r = np.random.default_rng(seed)
            pc = (T[:, :3] @ P.T).T + T[:, 3]
            k = np.zeros(n, api.KP_DTYPE)
            k["x"] = FX * pc[:, 0] / pc[:, 2] + CX + r.normal(0, 0.4, n); k["y"] = FY * pc[:, 1] / pc[:, 2] + CY + r.normal(0, 0.4, n)
            k["octave"] = r.integers(0, 8, n); k["angle"] = (base[1] + r.normal(0, 4, n)) % 360; k["size"] = 31; k["class_id"] = -1
            d = base[0] ^ np.packbits(r.random((n, 256)) < 0.03, axis=1, bitorder="little")
            ur = np.where(r.random(n) < 0.5, k["x"] - 40.0 / pc[:, 2], -1.0).astype(np.float32)
            has_mp = (r.random(n) < 0.3).astype(np.uint8)
            _, _, fv = TB._oracle_transform(L, v, d)
            return _kf(k, d, ur, has_mp, fv)

        _CACHE[("tv_base", n)] = dict(view=view, T1=T1, T2=T2)
    return _CACHE[("tv_base", n)]


def view_of(seed, n=1400):
    """KF2's pose seen with another seed: the neighbours of the CreateNewMapPoints loop."""
    key = ("view", seed, n)
    if key not in _CACHE:
        b = _two_view_base(n)
        _CACHE[key] = b["view"](b["T2"], seed)
    return _CACHE[key]


def two_view(seed2=2, n=1400):
    """n = 1400 is the scene of the tests; tools/bench_matchers.py --triangulation draws 2000 points."""
    key = ("two_view", seed2, n)
    if key not in _CACHE:
        b = _two_view_base(n)
        if ("tv_kf1", n) not in _CACHE:
            _CACHE[("tv_kf1", n)] = b["view"](b["T1"], 1)
        F12, Cw1, T2w = _f12(b["T1"], b["T2"])
        _CACHE[key] = dict(kf1=_CACHE[("tv_kf1", n)], kf2=view_of(seed2, n), F12=F12, Cw1=Cw1, T2w=T2w)
    return _CACHE[key]


# ------------------------------------------------------------------ big nodes
def _flip(rng, d, nbits):
    """Descriptor d with exactly nbits bits flipped."""
    out = np.unpackbits(d)
    out[rng.choice(256, nbits, replace=False)] ^= 1
    return np.packbits(out)


def big_node(seed=77):
    key = ("big", seed)
    if key in _CACHE:
        return _CACHE[key]
    from orbslam2_amd import api
    rng = np.random.default_rng(seed)
    ids = sorted(BIG_LAYOUT)
    n1 = sum(BIG_LAYOUT[i][0] for i in ids); n2 = sum(BIG_LAYOUT[i][1] for i in ids)
    assert (n1, n2) == (306, 4487)

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
    T1 = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    R2, t2 = _yaw(2.0), np.array([-0.05, 0.01, -0.4])
    T2 = np.concatenate([R2, t2[:, None]], axis=1)
    F12, Cw1, T2w = _f12(T1, T2)
    e2 = np.array([FX * t2[0] / t2[2] + CX, FY * t2[1] / t2[2] + CY])  # near (382, 228)

    def to_kf1(uv2, z2):
        pc2 = z2 * np.array([(uv2[0] - CX) / FX, (uv2[1] - CY) / FY, 1.0])
        pw = R2.T @ (pc2 - t2)
        return np.array([FX * pw[0] / pw[2] + CX, FY * pw[1] / pw[2] + CY])

    # KF2 starts as filler: random places, descriptors ~128 bits from everything
    k2 = np.zeros(n2, api.KP_DTYPE)
    k2["x"] = rng.uniform(20, 620, n2); k2["y"] = rng.uniform(20, 460, n2); k2["octave"] = rng.integers(0, 8, n2)
    k2["angle"] = rng.uniform(0, 359.9, n2); k2["size"] = 31; k2["class_id"] = -1
    d2 = rng.integers(0, 256, (n2, 32)).astype(np.uint8)
    ur2 = np.where(rng.random(n2) < 0.4, k2["x"] - 3.0, -1.0).astype(np.float32)
    mp2 = (rng.random(n2) < 0.15).astype(np.uint8)
    k1 = np.zeros(n1, api.KP_DTYPE)
    k1["octave"] = rng.integers(0, 8, n1); k1["angle"] = rng.uniform(0, 359.9, n1); k1["size"] = 31; k1["class_id"] = -1
    d1 = rng.integers(0, 256, (n1, 32)).astype(np.uint8)
    ur1 = np.full(n1, -1.0, np.float32)
    mp1 = (rng.random(n1) < 0.2).astype(np.uint8)
    uv2_of = np.zeros((n1, 2))
    node2_at = {int(nid): b for b, nid in enumerate(fv2[0])}

    def put_twin(idx1, idx2, dist_bits, uv, off_line, random_angle):
        """KF2 keypoint idx2 becomes a twin of KF1 keypoint idx1 at uv, optionally 40 px off idx1's epipolar line."""
        d2[idx2] = _flip(rng, d1[idx1], dist_bits)
        x, y = uv
        if off_line:
            a = k1["x"][idx1] * F12[0, 0] + k1["y"][idx1] * F12[1, 0] + F12[2, 0]
            b = k1["x"][idx1] * F12[0, 1] + k1["y"][idx1] * F12[1, 1] + F12[2, 1]
            nrm = np.hypot(a, b)
            x += 40.0 * a / nrm; y += 40.0 * b / nrm
        k2["x"][idx2] = x; k2["y"][idx2] = y
        k2["angle"][idx2] = rng.uniform(0, 359.9) if random_angle else (k1["angle"][idx1] + rng.normal(0, 4)) % 360
        if k2["angle"][idx2] >= 360:
            k2["angle"][idx2] = 0

    far_done = disc_done = 0
    for a, nid in enumerate(fv1[0]):
        seg1 = fv1[2][fv1[1][a]:fv1[1][a + 1]]
        b = node2_at.get(int(nid))
        seg2 = fv2[2][fv2[1][b]:fv2[1][b + 1]] if b is not None else np.zeros(0, np.int32)
        pool = rng.permutation(len(seg2)).tolist()           # free list positions of the KF2 node
        far = [p for p in pool if p >= 4096]                 # ... and those beyond the 64 flag bits of a lane
        pool = [p for p in pool if p < 4096]
        for i, idx1 in enumerate(seg1):
            forced_far = int(nid) == 20 and i % 4 == 2 and far_done < 12  # its duplicate, i + 1, then meets a flag beyond the lane's 64
            forced_disc = int(nid) == 8 and i % 4 == 0 and disc_done < 10
            if i % 4 == 3:                                   # duplicates its predecessor in descriptor and position
                prev = seg1[i - 1]
                d1[idx1] = d1[prev]; k1["x"][idx1] = k1["x"][prev]; k1["y"][idx1] = k1["y"][prev]; uv2_of[idx1] = uv2_of[prev]
            else:
                near = forced_disc or (not forced_far and rng.random() < 0.2)
                if near:                                     # projects close to the epipole of KF2
                    r, phi = (rng.uniform(1.5, 5.0) if forced_disc else rng.uniform(1.5, 15.0)), rng.uniform(0, 2 * np.pi)
                    uv2 = e2 + r * np.array([np.cos(phi), np.sin(phi)])
                else:
                    uv2 = np.array([rng.uniform(30, 610), rng.uniform(30, 450)])
                    while np.hypot(*(uv2 - e2)) < 40:
                        uv2 = np.array([rng.uniform(30, 610), rng.uniform(30, 450)])
                uv2_of[idx1] = uv2
                k1["x"][idx1], k1["y"][idx1] = to_kf1(uv2, rng.uniform(4, 30))
            ur1[idx1] = k1["x"][idx1] - 3.0 if rng.random() < 0.4 else -1.0
            if len(seg2) == 0:
                continue
            uv2 = uv2_of[idx1]
            if forced_disc:
                # a monocular twin at distance 0 inside the disc and a more distant alternative on the same epipolar line (it passes
                # through the epipole) outside every level's disc: the disc gate changes the winner
                mp1[idx1] = 0; ur1[idx1] = -1.0
                if len(pool) < 2:
                    continue
                direction = (uv2 - e2) / np.hypot(*(uv2 - e2))
                for dist_bits, uv in ((0, uv2), (8, e2 + 40.0 * direction)):
                    idx2 = seg2[pool.pop()]
                    put_twin(idx1, idx2, dist_bits, uv, False, False)
                    mp2[idx2] = 0; ur2[idx2] = -1.0
                disc_done += 1
                continue
            shared = rng.choice([0, 3, 8, 11, 50, 51], p=[0.3, 0.2, 0.15, 0.15, 0.1, 0.1])
            shared_desc = _flip(rng, d1[idx1], int(shared))
            for _ in range(int(rng.integers(1, 4))):
                if not pool:
                    break
                idx2 = seg2[pool.pop()]
                put_twin(idx1, idx2, 0, uv2 + rng.normal(0, 0.3, 2), rng.random() < 0.3, rng.random() < 0.2)
                if rng.random() < 0.7:                       # most twins of one feature are identical
                    d2[idx2] = shared_desc
                else:
                    d2[idx2] = _flip(rng, d1[idx1], int(rng.choice([0, 3, 8, 11, 50, 51])))
            if forced_far and far:
                # a distance-0 twin beyond list position 4096, usable, on the line, away from the epipole: the last of the equal minima
                mp1[idx1] = 0
                idx2 = seg2[far.pop()]
                put_twin(idx1, idx2, 0, uv2, False, False)
                mp2[idx2] = 0
                far_done += 1
    assert far_done >= 8 and disc_done >= 8
    out = dict(kf1=_kf(k1, d1, ur1, mp1, fv1), kf2=_kf(k2, d2, ur2, mp2, fv2), F12=F12, Cw1=Cw1, T2w=T2w, epipole=e2)
    _CACHE[key] = out
    return out


def single_node(n1, n2, seed=5):
    """One shared node, identical descriptors throughout, every KF2 keypoint on every epipolar line's acceptance band: each step is a
    tie of all free KF2 keypoints and takes a flag."""
    from orbslam2_amd import api
    sc = big_node()
    rng = np.random.default_rng(seed)
    desc = rng.integers(0, 256, 32).astype(np.uint8)

    def kf(n, x, y):
        k = np.zeros(n, api.KP_DTYPE)
        k["x"] = x; k["y"] = y; k["octave"] = 0; k["angle"] = 10.0; k["size"] = 31; k["class_id"] = -1
        fv = (np.array([5], np.uint32), np.array([0, n], np.int32), np.arange(n, dtype=np.int32))
        return _kf(k, np.tile(desc, (n, 1)), np.full(n, -1.0, np.float32), np.zeros(n, np.uint8), fv)

    # one KF1 place and its exact image in KF2 for all: the same epipolar line, all candidates on it and far from the epipole
    uv2 = np.array([150.0, 300.0])
    pc2 = 10.0 * np.array([(uv2[0] - CX) / FX, (uv2[1] - CY) / FY, 1.0])
    T2 = sc["T2w"].astype(np.float64)
    pw = T2[:, :3].T @ (pc2 - T2[:, 3])
    x1, y1 = FX * pw[0] / pw[2] + CX, FY * pw[1] / pw[2] + CY
    return dict(kf1=kf(n1, x1, y1), kf2=kf(n2, uv2[0], uv2[1]), F12=sc["F12"], Cw1=sc["Cw1"], T2w=sc["T2w"])


# ------------------------------------------------------------------ oracle
def oracle(sc, only_stereo, check_ori, mp1=None):
    """orc_search_for_triangulation on a scene: (match12, count)."""
    L = O.lib()
    L.orc_search_for_triangulation.restype = C.c_int
    L.orc_search_for_triangulation.argtypes = ([C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 4 + [C.c_int]) * 2 + [C.c_void_p] * 3 + \
        [C.c_float] * 4 + [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    a, b = sc["kf1"], sc["kf2"]
    sf, s2 = levels()
    mp1 = a["mp"] if mp1 is None else np.ascontiguousarray(mp1, np.uint8)
    n1, n2 = len(a["k"]), len(b["k"])
    ref = np.zeros(max(n1, 1), np.int32)
    nref = L.orc_search_for_triangulation(_p(a["fv"][0]), _p(a["fv"][1]), _p(a["fv"][2]), len(a["fv"][0]), _p(a["k"]), _p(a["ur"]), _p(mp1), _p(a["d"]), n1,
                                          _p(b["fv"][0]), _p(b["fv"][1]), _p(b["fv"][2]), len(b["fv"][0]), _p(b["k"]), _p(b["ur"]), _p(b["mp"]), _p(b["d"]), n2,
                                          _p(sc["F12"]), _p(sc["Cw1"]), _p(sc["T2w"]), FX, FY, CX, CY, _p(sf), _p(s2), int(only_stereo), int(check_ori), _p(ref))
    return ref[:n1].copy(), nref


def pairs_of(match12):
    """vMatchedPairs (:808-816): (idx1, idx2) of the non-negative entries in ascending idx1, flattened."""
    i1 = np.nonzero(match12 >= 0)[0]
    return np.stack([i1, match12[i1]], axis=1).astype(np.int32).reshape(-1)


# ------------------------------------------------------------------ census
def _rot_bin(a1, a2):
    rot = np.float32(a1) - np.float32(a2)
    if rot < 0.0:
        rot = np.float32(rot + np.float32(360.0))
    b = int(np.floor(float(np.float32(rot * np.float32(1.0 / HISTO_LENGTH))) + 0.5))  # roundf of a value >= 0
    return 0 if b == HISTO_LENGTH else b


def _three_maxima(sizes):
    order = sorted((i for i in range(len(sizes)) if sizes[i] > 0), key=lambda i: (-sizes[i], i))[:3]
    ind = order + [-1] * (3 - len(order))
    val = [sizes[i] if i >= 0 else 0 for i in ind]
    if np.float32(val[1]) < np.float32(0.1) * np.float32(val[0]):
        ind[1] = ind[2] = -1
    elif np.float32(val[2]) < np.float32(0.1) * np.float32(val[0]):
        ind[2] = -1
    return ind


def census(sc, only_stereo, check_ori):
    """The loop of :676-806 with its gates as arrays over a node's KF2 list, and what each gate, the flags and the tie rule did to the
    winner.  Returns (match12, count, classes)."""
    a, b = sc["kf1"], sc["kf2"]
    sf, s2 = levels()
    F = sc["F12"].astype(np.float32); Cw1, T = sc["Cw1"], sc["T2w"]
    f32 = np.float32
    C2 = [f32(f32(f32(T[i, 0] * Cw1[0]) + f32(T[i, 1] * Cw1[1])) + f32(T[i, 2] * Cw1[2])) + T[i, 3] for i in range(3)]
    invz = f32(1.0) / C2[2]
    ex = f32(f32(f32(FX) * C2[0]) * invz) + f32(CX); ey = f32(f32(f32(FY) * C2[1]) * invz) + f32(CY)
    n1, n2 = len(a["k"]), len(b["k"])
    bits1, bits2 = np.unpackbits(a["d"], axis=1), np.unpackbits(b["d"], axis=1)
    match12 = np.full(n1, -1, np.int32)
    matched2 = np.zeros(n2, bool)
    cls = dict(pos64=0, pos128=0, pos4096=0, ties=0, flag_changed=0, line_changed=0, disc_changed=0, dist50=0, pruned=0)
    hist = [[] for _ in range(HISTO_LENGTH)]
    at2 = {int(nid): j for j, nid in enumerate(b["fv"][0])}

    def pick(mask, d):
        """Last of the smallest distances <= TH_LOW among mask, or -1: what `dist > bestDist` -> continue leaves."""
        ok = np.nonzero(mask & (d <= TH_LOW))[0]
        if len(ok) == 0:
            return -1
        return int(ok[np.nonzero(d[ok] == d[ok].min())[0][-1]])

    for i, nid in enumerate(a["fv"][0]):
        j = at2.get(int(nid))
        if j is None:
            continue
        seg2 = b["fv"][2][b["fv"][1][j]:b["fv"][1][j + 1]]
        x2, y2 = b["k"]["x"][seg2], b["k"]["y"][seg2]
        oct2 = b["k"]["octave"][seg2]
        stereo2 = b["ur"][seg2] >= 0
        usable2 = (b["mp"][seg2] == 0) & (stereo2 if only_stereo else True)
        dx, dy = ex - x2, ey - y2
        in_disc = dx * dx + dy * dy < f32(100) * sf[oct2]
        for idx1 in a["fv"][2][a["fv"][1][i]:a["fv"][1][i + 1]]:
            stereo1 = a["ur"][idx1] >= 0
            if a["mp"][idx1] or (only_stereo and not stereo1):
                continue
            d = (bits1[idx1][None, :] ^ bits2[seg2]).sum(axis=1)
            x1, y1 = a["k"]["x"][idx1], a["k"]["y"][idx1]
            la = x1 * F[0, 0] + y1 * F[1, 0] + F[2, 0]; lb = x1 * F[0, 1] + y1 * F[1, 1] + F[2, 1]; lc = x1 * F[0, 2] + y1 * F[1, 2] + F[2, 2]
            num = la * x2 + lb * y2 + lc
            den = la * la + lb * lb
            with np.errstate(divide="ignore", invalid="ignore"):
                dsqr = num * num / den
            on_line = (den != 0) & (dsqr.astype(np.float64) < 3.84 * s2[oct2].astype(np.float64))
            disc = in_disc & ~stereo2 if not stereo1 else np.zeros(len(seg2), bool)
            free = ~matched2[seg2]
            w = pick(usable2 & free & ~disc & on_line, d)
            cls["flag_changed"] += pick(usable2 & ~disc & on_line, d) != w
            cls["line_changed"] += pick(usable2 & free & ~disc, d) != w
            cls["disc_changed"] += pick(usable2 & free & on_line, d) != w
            if w < 0:
                continue
            passers = usable2 & free & ~disc & on_line & (d == d[w])
            cls["ties"] += int(passers[:w].any())
            cls["pos64"] += w >= 64; cls["pos128"] += w >= 128; cls["pos4096"] += w >= 4096; cls["dist50"] += int(d[w]) == TH_LOW
            match12[idx1] = seg2[w]; matched2[seg2[w]] = True
            if check_ori:
                hist[_rot_bin(a["k"]["angle"][idx1], b["k"]["angle"][seg2[w]])].append(idx1)
    if check_ori:
        keep = _three_maxima([len(h) for h in hist])
        for bin_, h in enumerate(hist):
            if bin_ not in keep:
                match12[h] = -1
                cls["pruned"] += len(h)
    return match12, int((match12 >= 0).sum()), {k: int(v) for k, v in cls.items()}
