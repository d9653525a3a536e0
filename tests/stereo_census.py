"""Census of Frame::ComputeStereoMatches' tail (reference src/Frame.cc:464-642): a plain NumPy restatement of the function as
written, which also counts which way every decision went, and the inputs that are built to reach each branch.

The restatement shares no code with oracle/orb_oracle.c.  It reads the same pyramids, keypoints and descriptors (two
oracle.Extractor objects after extract()), uses float32 scalars wherever the reference computes in float, and double for the
SAD accumulation (cv::norm) and for the 0.01 clamp.  tests/test_stereo_census.py holds it against O.stereo_matches bit for bit,
which is what makes the counters trustworthy; tests/test_gpu_stereo_tail.py runs the same inputs through the HIP path.

Two places cannot be restated as written, because the reference leaves them undefined; both follow the project's contract:
  * rows of the row table outside [0, nRows) are not written (the reference would write out of range);
  * Q2, an empty vDistIdx skips the median cut; Q12, a right band that starts left of the level image leaves the keypoint
    unmatched (cv::Mat::colRange would throw).
"""
from __future__ import annotations

import numpy as np

from oracle import oracle as O
from orbslam2_amd import synth

F = np.float32
TH_HIGH, TH_LOW = 100, 50
INT_MAX = 2 ** 31 - 1
_POP = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(axis=1).astype(np.int32)


def _round(x):
    """C round() of a non-negative float32 (half away from zero), as float32: exact in double."""
    return F(np.floor(float(x) + 0.5))


def census(exL, exR, kL, dL, kR, dR, bf, fx, trace=None):
    """(u_right, depth, counters) of one stereo pair; exL / exR hold the pair's pyramids.  trace: a list that receives
    (iL, uL, uR0, disparity) of every keypoint that gets as far as the disparity test."""
    N, Nr = len(kL), len(kR)
    u_right = np.full(N, -1.0, F)
    depth = np.full(N, -1.0, F)
    c = dict(n_left=N, n_right=Nr, coarse=0, hamming_tie=0, q12_guard=0, band_right_of_level=0, best_inc_at_end=0, sad_tie=0,
             delta_half=0, delta_min=None, delta_max=None, delta_denominator_zero=0, delta_outside_unit=0, disparity_negative=0,
             clamp=0, disparity_ge_maxd=0, disparity_eq_maxd=0, candidate_at_min_u=0, candidate_at_max_u=0,
             best_at_min_u=0, best_at_max_u=0, sad_at_threshold=0, accepted=0, nvdi=0, median=None, cut=0, clamp_surviving=0, matched=0, sad_max=0)
    th_orb_dist = (TH_HIGH + TH_LOW) // 2
    scale, inv_scale = exL.scale_factors(), exL.inv_scale_factors()
    pyrL = [exL.pyramid_level(l) for l in range(exL.nlevels)]
    pyrR = [exR.pyramid_level(l) for l in range(exR.nlevels)]
    n_rows = pyrL[0].shape[0]

    rows = [[] for _ in range(n_rows)]  # vRowIndices, :474-491
    for iR in range(Nr):
        kp_y = F(kR["y"][iR])
        r = F(2.0) * scale[kR["octave"][iR]]
        maxr, minr = int(np.ceil(kp_y + r)), int(np.floor(kp_y - r))
        for yi in range(max(minr, 0), min(maxr, n_rows - 1) + 1):
            rows[yi].append(iR)
    rows = [np.array(r, np.int64) for r in rows]

    mb = F(bf) / F(fx)  # Q1: mb := mbf / fx
    if mb == 0:  # :494
        return u_right, depth, c
    min_d, max_d = F(0), F(bf) / mb
    oct_r, x_r = kR["octave"].astype(np.int64), kR["x"].astype(F)
    dist_idx = []
    clamped = set()
    deltas = []
    for iL in range(N):
        level = int(kL["octave"][iL])
        vL, uL = F(kL["y"][iL]), F(kL["x"][iL])
        cand = rows[int(vL)]
        if len(cand) == 0:
            continue
        min_u, max_u = uL - max_d, uL - min_d
        if max_u < 0:
            continue
        # first minimum below TH_HIGH over the candidates that pass the octave and the disparity window, :530-551
        ok = (oct_r[cand] >= level - 1) & (oct_r[cand] <= level + 1)
        c["candidate_at_min_u"] += int((ok & (x_r[cand] == min_u)).any())
        c["candidate_at_max_u"] += int((ok & (x_r[cand] == max_u)).any())
        ok &= (x_r[cand] >= min_u) & (x_r[cand] <= max_u)
        cand = cand[ok]
        best_dist, best_r = TH_HIGH, 0
        if len(cand):
            d = _POP[dL[iL][None, :] ^ dR[cand]].sum(axis=1)
            j = int(np.argmin(d))  # the first of equal minima, like `dist < bestDist`
            if d[j] < best_dist:
                best_dist, best_r = int(d[j]), int(cand[j])
        if not best_dist < th_orb_dist:
            continue
        c["coarse"] += 1
        c["hamming_tie"] += int((d == best_dist).sum() > 1)
        uR0 = x_r[best_r]
        c["best_at_min_u"] += int(uR0 == min_u)
        c["best_at_max_u"] += int(uR0 == max_u)
        sf = inv_scale[level]
        s_uL, s_vL, s_uR0 = _round(uL * sf), _round(vL * sf), _round(uR0 * sf)
        w, L = 5, 5
        cu, cv, cr = int(s_uL), int(s_vL), int(s_uR0)
        imL, imR = pyrL[level], pyrR[level]
        cols = imR.shape[1]
        IL = imL[cv - w:cv + w + 1, cu - w:cu + w + 1].astype(F)
        assert IL.shape == (11, 11), "left window outside its level: keypoint %d" % iL
        IL = IL - IL[w, w]
        iniu, endu = s_uR0 + F(L) - F(w), s_uR0 + F(L) + F(w) + F(1)
        if iniu < 0 or endu >= cols:
            c["band_right_of_level"] += int(endu >= cols)
            continue
        if cr - L - w < 0:  # Q12
            c["q12_guard"] += 1
            continue
        if cr + L + w >= cols:  # cannot happen: see test_stereo_census.test_dead_branches
            c["band_right_of_level"] += 1
            continue
        sad_best, best_inc = INT_MAX, 0
        dists = np.zeros(2 * L + 1, F)
        for inc in range(-L, L + 1):
            IR = imR[cv - w:cv + w + 1, cr + inc - w:cr + inc + w + 1].astype(F)
            IR = IR - IR[w, w]
            dist = F(np.abs(IL - IR).astype(np.float64).sum())  # cv::norm(NORM_L1) of CV_32F sums in double
            if dist < F(sad_best):
                sad_best, best_inc = int(dist), inc
            dists[L + inc] = dist
        c["sad_max"] = max(c["sad_max"], int(dists.max()))
        c["sad_tie"] += int((dists == dists.min()).sum() > 1)
        if best_inc == -L or best_inc == L:
            c["best_inc_at_end"] += 1
            continue
        d1, d2, d3 = dists[L + best_inc - 1], dists[L + best_inc], dists[L + best_inc + 1]
        den = F(2.0) * (d1 + d3 - F(2.0) * d2)
        if den == 0:
            c["delta_denominator_zero"] += 1
        with np.errstate(divide="ignore", invalid="ignore"):
            delta_r = (d1 - d3) / den
        deltas.append(delta_r)
        c["delta_half"] += int(delta_r == F(0.5))
        if delta_r < -1 or delta_r > 1 or delta_r != delta_r:
            c["delta_outside_unit"] += 1
            if delta_r == delta_r:
                continue
        best_ur = scale[level] * (s_uR0 + F(best_inc) + delta_r)
        disparity = uL - best_ur
        c["disparity_negative"] += int(disparity < min_d)
        c["disparity_ge_maxd"] += int(disparity >= max_d)
        c["disparity_eq_maxd"] += int(disparity == max_d)
        if trace is not None:
            trace.append((iL, float(uL), float(uR0), float(disparity)))
        if disparity >= min_d and disparity < max_d:
            if disparity <= 0:
                disparity = F(0.01)
                best_ur = F(np.float64(uL) - 0.01)
                c["clamp"] += 1
                clamped.add(iL)
            depth[iL] = F(bf) / disparity
            u_right[iL] = best_ur
            dist_idx.append((sad_best, iL))
            c["accepted"] += 1

    c["nvdi"] = len(dist_idx)
    if deltas:
        c["delta_min"], c["delta_max"] = float(min(deltas)), float(max(deltas))
    if dist_idx:  # :628-641; Q2
        dist_idx.sort()
        median = F(dist_idx[len(dist_idx) // 2][0])
        c["median"] = int(median)
        th_dist = F(1.5) * F(1.4) * median
        c["sad_at_threshold"] = sum(1 for sad, _ in dist_idx if F(sad) == th_dist)
        for sad, iL in reversed(dist_idx):
            if F(sad) < th_dist:
                break
            u_right[iL] = -1
            depth[iL] = -1
            clamped.discard(iL)
            c["cut"] += 1
    c["clamp_surviving"] = len(clamped)
    c["matched"] = int((u_right >= 0).sum())
    return u_right, depth, c


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
W, H = 640, 360
BASE = dict(width=W, height=H, nfeatures=1000, fx=384.0, fy=384.0, cx=W / 2, cy=H / 2, bf=160.0)


def _cfg(w, h, nf, fx, bf, **kw):
    return dict(width=w, height=h, nfeatures=nf, fx=float(fx), fy=float(fx), cx=w / 2, cy=h / 2, bf=float(bf), **kw)


def checkerboard(w, h, square):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where(((xx // square) + (yy // square)) % 2 == 0, 225, 30).astype(np.uint8)


def _synth(cfg, seed):
    return synth.stereo_pair(cfg["width"], cfg["height"], seed=seed)


def _noisy_copy(seed=5):
    left = _synth(BASE, seed)[0]
    noise = np.random.default_rng(seed).integers(-3, 4, left.shape)
    return left, np.clip(left.astype(np.int32) + noise, 0, 255).astype(np.uint8)


def _composite(seed, square, x0, x1, y0, y1):
    left, right = (a.copy() for a in _synth(BASE, seed))
    block = checkerboard(W, H, square)[y0:y1, x0:x1]
    left[y0:y1, x0:x1] = block
    right[y0:y1, x0:x1] = block
    return left, right


def _textured_flat(seed=5):
    left = _synth(BASE, seed)[0]
    return left, np.full_like(left, 120)


KITTI = dict(width=1241, height=376, nfeatures=2000, fx=718.856, fy=718.856, cx=607.1928, cy=185.2157, bf=386.1448)
SMALL = dict(width=320, height=240, nfeatures=500, fx=300.0, fy=300.0, cx=160.0, cy=120.0, bf=120.0)
EUROC = dict(width=752, height=480, nfeatures=1200, fx=458.654, fy=457.296, cx=367.215, cy=248.375, bf=47.9)
CHECKER = _cfg(752, 480, 1200, 460.0, 50.0)
Q12 = _cfg(451, 278, 729, 0.7 * 451, 0.2 * 451, ini_th_fast=33, min_th_fast=19,
           scale_factor=float(np.float32(2.218409776687622)), nlevels=6)


def _rolled_checker(square, shift):
    left = checkerboard(752, 480, square)
    return left, np.roll(left, shift, axis=1)


def _maxd(fx):
    return dict(BASE, fx=fx, fy=fx, bf=float(np.float32(0.4) * np.float32(fx)))


# name -> (config, builder of (left, right), the branch the input is there for)
INPUTS = {
    # inputs the GPU suite already had (test_gpu_parity, test_gpu_sweep): on record next to the new ones
    "kitti": (KITTI, lambda: _synth(KITTI, 1234), "existing input"),
    "small": (SMALL, lambda: _synth(SMALL, 1234), "existing input"),
    "euroc": (EUROC, lambda: _synth(EUROC, 1234), "existing input"),
    "777x333": (_cfg(777, 333, 1500, 0.6 * 777, 0.25 * 777), lambda: synth.stereo_pair(777, 333, seed=1), "existing input"),
    "131x97": (_cfg(131, 97, 200, 0.6 * 131, 0.25 * 131), lambda: synth.stereo_pair(131, 97, seed=6), "existing input: even nvdi below 16"),
    "checker24_roll9": (CHECKER, lambda: _rolled_checker(24, -9), "existing input: SAD ties, bestincR at the band's end"),
    "q12": (Q12, lambda: synth.stereo_pair(451, 278, seed=131000 + 2000 + 329), "existing input: Q12 guard"),
    # new
    "noisy_copy": (BASE, _noisy_copy, "disparity < 0 next to accepted matches"),
    "roll_plus1": (BASE, lambda: (lambda l: (l, np.roll(l, 1, axis=1)))(_synth(BASE, 5)[0]), "disparity < 0"),
    "maxd_11.5": (_maxd(11.5), lambda: _synth(BASE, 6), "disparity >= maxD"),
    "maxd_27.75": (_maxd(27.75), lambda: _synth(BASE, 6), "disparity >= maxD"),
    "maxd_61": (_maxd(61.0), lambda: _synth(BASE, 6), "disparity >= maxD"),
    "identical": (BASE, lambda: (lambda l: (l, l.copy()))(_synth(BASE, 5)[0]), "median 0: every accepted match is cut"),
    "checker24_identical": (CHECKER, lambda: _rolled_checker(24, 0), "0.01 clamp, erased again by a median of 0"),
    "composite5": (BASE, lambda: _composite(5, 24, 40, 300, 60, 300), "0.01 clamp that survives the median cut"),
    "composite6": (BASE, lambda: _composite(6, 37, 300, 620, 20, 340), "0.01 clamp that survives the median cut"),
    "composite7": (BASE, lambda: _composite(7, 16, 100, 400, 100, 260), "0.01 clamp that survives the median cut"),
    "bf0": (dict(BASE, bf=0.0), lambda: _synth(BASE, 5), "bf == 0: the search is skipped"),
    "right_flat": (BASE, _textured_flat, "no accepted match: the median cut is skipped"),
    "ordinary6": (BASE, lambda: _synth(BASE, 6), "ordinary pair on the batch geometry"),
    "ordinary7": (BASE, lambda: _synth(BASE, 7), "ordinary pair on the batch geometry"),
    "maxd_equal": (dict(BASE, fx=28.4320068359375, fy=28.4320068359375, bf=11.372802734375), lambda: _synth(BASE, 6),
                   "disparity == maxD exactly (both float32 values as written)"),
    "window_edge": (dict(BASE, fx=28.0, fy=28.0, bf=14.0), lambda: _synth(BASE, 6), "right keypoints exactly at uL - maxD, the window's lower bound"),
    "threshold_equal": (BASE, lambda: _synth(BASE, 1055), "an accepted SAD equal to 1.5 * 1.4 * median: cut by `<`"),
    "checker37_roll9_dense": (dict(CHECKER, nfeatures=3000), lambda: _rolled_checker(37, -9), "Hamming ties, SAD ties, delta_r == 0.5"),
    "131x97_odd": (_cfg(131, 97, 200, 0.6 * 131, 0.25 * 131), lambda: synth.stereo_pair(131, 97, seed=1234), "odd nvdi below 16, two cut"),
    "96x64_single": (_cfg(96, 64, 100, 0.6 * 96, 0.25 * 96), lambda: synth.stereo_pair(96, 64, seed=2), "nvdi == 1: the median is the only match"),
}

# one batched call on the BASE geometry: ordinary, median 0, no match at all, clamp survives, ordinary
BATCH = ("ordinary6", "identical", "right_flat", "composite5", "ordinary7")

EXTRACTOR_KEYS = ("nfeatures", "scale_factor", "nlevels", "ini_th_fast", "min_th_fast")


def extractor_kwargs(cfg):
    return {k: cfg[k] for k in EXTRACTOR_KEYS if k in cfg}


def build(name):
    """(config, left, right, branch) of a census input."""
    cfg, make, branch = INPUTS[name]
    left, right = make()
    return cfg, np.ascontiguousarray(left), np.ascontiguousarray(right), branch


def oracle_frame(cfg, left, right):
    """The oracle's extraction of a pair: (exL, exR, kL, dL, kR, dR)."""
    exl, exr = O.Extractor(**extractor_kwargs(cfg)), O.Extractor(**extractor_kwargs(cfg))
    kl, dl = exl.extract(left)
    kr, dr = exr.extract(right)
    return exl, exr, kl, dl, kr, dr


GOLDEN = "stereo_tail_census.json"  # under tests/golden/


def census_of(name):
    """(oracle u_right, oracle depth, restated u_right, restated depth, counters) of a census input."""
    cfg, left, right, _ = build(name)
    exl, exr, kl, dl, kr, dr = oracle_frame(cfg, left, right)
    ur, dp, _ = O.stereo_matches(exl, exr, kl, dl, kr, dr, cfg["bf"], cfg["fx"])
    u2, d2, c = census(exl, exr, kl, dl, kr, dr, cfg["bf"], cfg["fx"])
    return ur, dp, u2, d2, c


if __name__ == "__main__":  # python -m tests.stereo_census: rewrite the pinned table after a deliberate change of an input
    import json
    import os
    table = {name: census_of(name)[4] for name in INPUTS}
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN), "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
