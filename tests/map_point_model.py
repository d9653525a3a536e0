"""Literal model of MapPoint::ComputeDistinctiveDescriptors (reference src/MapPoint.cc:242-307) and MapPoint::UpdateNormalAndDepth
(:330-371) on Python lists, in the style of oracle/literal_*.py: the reference's loops line by line, every float step an explicit
np.float32 / np.float64 operation.  It is the reference of tests/test_map_point_model.py (against orbslam2_amd/host/MapPointUpdate.h)
and tests/test_map_point_device.py (against orbfe_enqueue_update_map_points).

Float contract (Q4 of oracle/orb_oracle_match.c, plus two OPENCV-4.5.5-SEMANTICS steps that DESIGN.md section 2 lists as unpinned):
  cv::norm(float vector)   tests/cvmat_model.py's norm(): double sum of double squares, left to right, one sqrt
  Mat / double             a scale by 1./s; `normal + that` is scaleAdd with the factor cast to float: (float)(d * alpha) + acc
  Mat / int                convertTo with the float scale (float)(1.0 / n): a product, not a division
"""
import numpy as np

from tests.cvmat_model import F32, F64, norm

INT_MAX = 2 ** 31 - 1
MP_DESCRIPTOR, MP_NORMAL_DEPTH = 1, 2
ERR_INVALID = -1


def as_int(desc):
    """32 descriptor bytes as one Python int (its bit count is the Hamming weight)."""
    return int.from_bytes(bytes(bytearray(desc)), "little")


def descriptor_distance(a, b):
    """ORBmatcher::DescriptorDistance on descriptors held as ints."""
    return (a ^ b).bit_count()


def compute_distinctive_descriptors(descs, bad):
    """descs: the observed descriptors as ints, in the order of mObservations; bad: pKF->isBad() per observation.
    Returns (list position of the chosen descriptor or -1 when mDescriptor is not written, best median, #entries sharing it)."""
    if len(descs) == 0:                       # :256-257
        return -1, None, 0
    vDescriptors, where = [], []
    for p in range(len(descs)):               # :261-267
        if not bad[p]:
            vDescriptors.append(descs[p])
            where.append(p)
    if len(vDescriptors) == 0:                # :269-270
        return -1, None, 0
    N = len(vDescriptors)
    Distances = [[0] * N for _ in range(N)]
    for i in range(N):                        # :276-285
        Distances[i][i] = 0
        for j in range(i + 1, N):
            distij = descriptor_distance(vDescriptors[i], vDescriptors[j])
            Distances[i][j] = distij
            Distances[j][i] = distij
    BestMedian, BestIdx, sharing = INT_MAX, 0, 0
    for i in range(N):                        # :290-301
        vDists = sorted(Distances[i])
        median = vDists[int(0.5 * (N - 1))]
        if median < BestMedian:
            BestMedian, BestIdx, sharing = median, i, 1
        elif median == BestMedian:
            sharing += 1                      # census only: how many entries tie for the best median
    return where[BestIdx], BestMedian, sharing


def update_normal_and_depth(pos, centres, ref, level, scale, nlevels, divide=False):
    """pos: mWorldPos (3 float32); centres: GetCameraCenter() per observation in the order of mObservations; ref: position of mpRefKF
    in that list; level: its keypoint's octave.  Returns (normal[3], mfMaxDistance, mfMinDistance) as np.float32.  divide=True is the
    variant the contract rules OUT (normal / n and normali / norm as true divisions), kept to show that the choice is visible."""
    pos = [F32(x) for x in pos]
    normal = [F32(0), F32(0), F32(0)]
    n = 0
    for Ow in centres:                        # :350-357
        normali = [pos[c] - F32(Ow[c]) for c in range(3)]
        nrm = norm(normali)
        if divide:
            normal = [F32(F64(normali[c]) / nrm) + normal[c] for c in range(3)]
        else:
            alpha = F32(F64(1.0) / nrm)
            normal = [F32(normali[c] * alpha) + normal[c] for c in range(3)]
        n += 1
    PC = [pos[c] - F32(centres[ref][c]) for c in range(3)]   # :359
    dist = F32(norm(PC))
    mfMaxDistance = dist * F32(scale[level])                  # :367
    mfMinDistance = mfMaxDistance / F32(scale[nlevels - 1])  # :368
    if divide:
        out = [normal[c] / F32(n) for c in range(3)]
    else:
        inv = F32(F64(1.0) / F64(n))
        out = [normal[c] * inv for c in range(3)]            # :369
    assert all(type(x) is F32 for x in out + [mfMaxDistance, mfMinDistance])
    return out, mfMaxDistance, mfMinDistance


def update_map_points(s, what, table, ignore_bad=False):
    """orbfe_enqueue_update_map_points on a scene of tests/map_point_scenes.py: rewrites the selected columns of `table` (a dict of
    numpy arrays: normal, max_d, min_d, desc) in place and returns (best[n_upd], status).  A faulty update (include/orbfe.h) is
    skipped whole and sets the status."""
    n_upd, status = len(s["obs_off"]) - 1, 0
    best = np.full(n_upd, -1, np.int32)
    n_kfs, n_rows, n_obs = len(s["kf_n"]), len(table["max_d"]), len(s["obs_kf"])
    for q in range(n_upd):
        r = int(s["row"][q]) if s["row"] is not None else q
        o0, o1 = int(s["obs_off"][q]), int(s["obs_off"][q + 1])
        fault = r < 0 or r >= n_rows or o0 < 0 or o1 < o0 or o1 > n_obs
        obs = [] if fault else [(int(s["obs_kf"][o]), int(s["obs_idx"][o])) for o in range(o0, o1)]
        fault = fault or any(kf < 0 or kf >= n_kfs or idx < 0 or idx >= s["kf_n"][kf] for kf, idx in obs)
        if not fault and (what & MP_NORMAL_DEPTH) and obs:
            ref = int(s["ref"][q])
            fault = ref < 0 or ref >= len(obs)
            if not fault:
                level = int(s["kf_octave"][obs[ref][0]][obs[ref][1]])
                fault = level < 0 or level >= s["nlevels"]
        if fault:
            status = ERR_INVALID
            continue
        if not obs:
            continue
        if what & MP_DESCRIPTOR:
            descs = [s["kf_desc_int"][kf][idx] for kf, idx in obs]
            bad = [0 if ignore_bad else int(s["kf_bad"][kf]) for kf, _ in obs]
            best[q], _, _ = compute_distinctive_descriptors(descs, bad)
            if best[q] >= 0:
                kf, idx = obs[best[q]]
                table["desc"][r] = s["kf_desc"][kf][idx]
        if what & MP_NORMAL_DEPTH:
            nrm, mx, mn = update_normal_and_depth(s["pos"][r], [s["Ow"][kf] for kf, _ in obs], ref, level, s["scale"], s["nlevels"])
            table["normal"][r] = nrm
            table["max_d"][r], table["min_d"][r] = mx, mn
    return best, status
