"""Literal model of the triangulation stage of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:286-450, with
KeyFrame::UnprojectStereo, src/KeyFrame.cc:609-625) on the flat arrays of orbfe_enqueue_triangulate_pairs (include/orbfe.h): the
reference's loop line by line, every float step an explicit np.float32 / np.float64 operation, Python loops, nothing vectorised.  It is
the reference of tests/test_triangulate_model.py (against orbslam2_amd/host/Triangulate.h) and tests/test_triangulate_device.py
(against the kernel); both must equal it bit for bit.  pair_f64() is the same branch structure in double with numpy.linalg.svd.

Float contract (Q4: no contraction, IEEE divide and sqrt; the OpenCV steps are OPENCV-4.5.5-SEMANTICS, unpinned as DESIGN.md section 2
says, and stated in sections 4i2 and 4k; the cv::Mat rules themselves are tests/cvmat_model.py's):
  xn                        ((x - cx) * invfx, (y - cy) * invfy, 1) in float
  Mat * Mat (3x3 * 3x1)     mat(): `Rwc * x3Dc + Ow` adds Ow in double before the one rounding
  Mat::dot, cv::norm        double sums in index order; norm() takes one double sqrt
  s * row - row             a float multiply, then a float subtract, per element
  Mat / float               a scale by (float)(1.0 / w): a product, not a division
  row.dot(x3Dt) + t         double dot + float in double, rounded to float
  cv::SVD -> vt.row(3)      null_vector(A): vt.row(3) and info = dict(sweeps, rotations, first_beta_negative (None: no rotation), swaps)
A keyframe is a dict: keys_un, keys (structured, x / y / octave), ur, depth, cos (float32[n]), mp (uint8[n], writable), n, Tcw
(float32[12]), Ow (float32[3]), fx, fy, cx, cy, invfx, invfy (np.float32).
"""
import numpy as np

from tests.cvmat_model import F32, F64, MAX_SWEEPS, mat, norm, null_vector  # noqa: F401 (MAX_SWEEPS is read through this module)

ERR_INVALID, ERR_CAPACITY = -1, -4
CREATED_MAX = 2          # a pair is created iff its code is <= 2
(TRIANGULATED, STEREO1, STEREO2, LOW_PARALLAX, W_ZERO, Z1, Z2, REPROJ1, REPROJ2, ZERO_DIST, SCALE, FAULTY) = range(12)
TRACE = None


# ------------------------------------------------------------------ cv::Mat steps (tests/cvmat_model.py's rules on a Tcw of 12 floats)
def _rwc_times(T, x, plus=None):
    """Rwc * x (+ Ow): Rwc = Rcw.t()."""
    Rcw = np.asarray(T, F32).reshape(3, 4)[:, :3]
    return mat(Rcw.T, np.asarray(x, F32)[:, None], plus=None if plus is None else np.asarray(plus, F32)[:, None])[:, 0]


def _row_dot_plus(T, r, X):
    """Rcw.row(r).dot(x3Dt) + tcw(r): the double dot plus the float, rounded to float."""
    T = np.asarray(T, F32).reshape(3, 4)
    return mat(T[r:r + 1, :3], np.asarray(X, F32)[:, None], plus=T[r:r + 1, 3:])[0, 0]


def _xn(kf, kp):
    return [F32(F32(kp["x"] - kf["cx"]) * kf["invfx"]), F32(F32(kp["y"] - kf["cy"]) * kf["invfy"]), F32(1)]


def unproject_stereo(kf, i):
    z = F32(kf["depth"][i])
    u, v = F32(kf["keys"]["x"][i]), F32(kf["keys"]["y"][i])
    x = F32(F32(F32(u - kf["cx"]) * z) * kf["invfx"])
    y = F32(F32(F32(v - kf["cy"]) * z) * kf["invfy"])
    return _rwc_times(kf["Tcw"], [x, y, z], plus=kf["Ow"])


def _reprojection_fails(kf, kp, ur, stereo, X, z, mbf, sigma2):
    x, y = _row_dot_plus(kf["Tcw"], 0, X), _row_dot_plus(kf["Tcw"], 1, X)
    invz = F32(F64(1.0) / F64(z))
    u = F32(F32(F32(kf["fx"] * x) * invz) + kf["cx"])
    v = F32(F32(F32(kf["fy"] * y) * invz) + kf["cy"])
    ex, ey = F32(u - kp["x"]), F32(v - kp["y"])
    e = F32(F32(ex * ex) + F32(ey * ey))
    if not stereo:
        return F64(e) > F64(5.991) * F64(sigma2)
    u_r = F32(u - F32(mbf * invz))
    er = F32(u_r - ur)
    e = F32(e + F32(er * er))
    return F64(e) > F64(7.8) * F64(sigma2)


def pair(kf1, kf2, idx1, idx2, mbf, ratio_factor, sf, s2):
    """One iteration of :286-450.  Returns (code, x3D as three np.float32 or None, info of null_vector or None)."""
    nlevels = len(sf)
    mbf, ratio_factor = F32(mbf), F32(ratio_factor)
    if idx1 < 0 or idx1 >= kf1["n"] or idx2 < 0 or idx2 >= kf2["n"]:
        return FAULTY, None, None
    kp1, kp2 = kf1["keys_un"][idx1], kf2["keys_un"][idx2]
    o1, o2 = int(kp1["octave"]), int(kp2["octave"])
    if o1 < 0 or o1 >= nlevels or o2 < 0 or o2 >= nlevels:
        return FAULTY, None, None
    ur1, ur2 = F32(kf1["ur"][idx1]), F32(kf2["ur"][idx2])
    stereo1, stereo2 = bool(ur1 >= 0), bool(ur2 >= 0)
    if (stereo1 and not kf1["depth"][idx1] > 0) or (stereo2 and not kf2["depth"][idx2] > 0):
        return FAULTY, None, None          # UnprojectStereo would return an empty Mat
    xn1, xn2 = _xn(kf1, kp1), _xn(kf2, kp2)
    ray1, ray2 = _rwc_times(kf1["Tcw"], xn1), _rwc_times(kf2["Tcw"], xn2)
    dot = F64(0)
    for k in range(3):
        dot = dot + F64(ray1[k]) * F64(ray2[k])
    cos_rays = F32(dot / (norm(ray1) * norm(ray2)))
    cos_stereo = F32(cos_rays + F32(1))
    cos1 = cos2 = cos_stereo
    if stereo1:
        cos1 = F32(kf1["cos"][idx1])
    elif stereo2:
        cos2 = F32(kf2["cos"][idx2])
    cos_stereo = cos2 if cos2 < cos1 else cos1   # std::min(cos1, cos2)
    info = None
    if cos_rays < cos_stereo and cos_rays > 0 and (stereo1 or stereo2 or F64(cos_rays) < F64(0.9998)):
        T1, T2 = kf1["Tcw"], kf2["Tcw"]
        A = [[F32(F32(xn1[0] * T1[8 + c]) - T1[c]) for c in range(4)],
             [F32(F32(xn1[1] * T1[8 + c]) - T1[4 + c]) for c in range(4)],
             [F32(F32(xn2[0] * T2[8 + c]) - T2[c]) for c in range(4)],
             [F32(F32(xn2[1] * T2[8 + c]) - T2[4 + c]) for c in range(4)]]
        v, info = null_vector(A)
        if v[3] == 0:
            return W_ZERO, None, info
        alpha = F32(F64(1.0) / F64(v[3]))
        X = [F32(v[0] * alpha), F32(v[1] * alpha), F32(v[2] * alpha)]
        code = TRIANGULATED
    elif stereo1 and cos1 < cos2:
        X, code = unproject_stereo(kf1, idx1), STEREO1
    elif stereo2 and cos2 < cos1:
        X, code = unproject_stereo(kf2, idx2), STEREO2
    else:
        return LOW_PARALLAX, None, None
    z1 = _row_dot_plus(kf1["Tcw"], 2, X)
    if z1 <= 0:
        return Z1, None, info
    z2 = _row_dot_plus(kf2["Tcw"], 2, X)
    if z2 <= 0:
        return Z2, None, info
    if _reprojection_fails(kf1, kp1, ur1, stereo1, X, z1, mbf, s2[o1]):
        return REPROJ1, None, info
    if _reprojection_fails(kf2, kp2, ur2, stereo2, X, z2, mbf, s2[o2]):
        return REPROJ2, None, info
    dist1 = F32(norm([F32(X[k] - kf1["Ow"][k]) for k in range(3)]))
    dist2 = F32(norm([F32(X[k] - kf2["Ow"][k]) for k in range(3)]))
    if dist1 == 0 or dist2 == 0:
        return ZERO_DIST, None, info
    ratio_dist = F32(dist2 / dist1)
    ratio_octave = F32(F32(sf[o1]) / F32(sf[o2]))
    if F32(ratio_dist * ratio_factor) < ratio_octave or ratio_dist > F32(ratio_octave * ratio_factor):
        return SCALE, None, info
    return code, X, info


# ------------------------------------------------------------------ the call
def triangulate_pairs(kf1, kf2, mbf, ratio_factor, pairs, npairs, max_pairs, sf, s2, code, x3d, new, pos=None, n_rows=0, rows_used=0, patch_has_mp=1):
    """orbfe_enqueue_triangulate_pairs on numpy arrays; code (uint8[max_pairs]), x3d (float32[max_pairs][3]), new (int32[3 * max_pairs]),
    pos (float32[n_rows][3] or None) and both mp arrays are written in place.  npairs is the device word.
    Returns dict(status, nnew (None: untouched), rows_used, infos)."""
    with np.errstate(all="ignore"):
        if max_pairs == 0:
            return dict(status=0, nnew=0, rows_used=rows_used, infos=[])
        if npairs < 0 or npairs > max_pairs:
            return dict(status=ERR_INVALID, nnew=None, rows_used=rows_used, infos=[])
        status, created, infos = 0, [], []
        for q in range(npairs):
            idx1, idx2 = int(pairs[2 * q]), int(pairs[2 * q + 1])
            c, X, info = pair(kf1, kf2, idx1, idx2, mbf, ratio_factor, sf, s2)
            infos.append(info)
            code[q] = c
            if c == FAULTY:
                status = ERR_INVALID
            if c <= CREATED_MAX:
                x3d[q] = X
                created.append(q)
        nnew = len(created)
        table = pos is not None
        if table and rows_used < 0:
            status, table = ERR_INVALID, False
            fits = False
        elif table and rows_used + nnew > n_rows:
            status, table = ERR_CAPACITY, False
            fits = False
        else:
            fits = True
        for k, q in enumerate(created):
            idx1, idx2 = int(pairs[2 * q]), int(pairs[2 * q + 1])
            row = rows_used + k if table else -1
            new[3 * k: 3 * k + 3] = (idx1, idx2, row)
            if table:
                pos[row] = x3d[q]
            if patch_has_mp and fits:
                kf1["mp"][idx1] = 1
                kf2["mp"][idx2] = 1
        return dict(status=status, nnew=nnew, rows_used=rows_used + nnew if table else rows_used, infos=infos)


# ------------------------------------------------------------------ the float64 restatement
def pair_f64(kf1, kf2, idx1, idx2, mbf, ratio_factor, sf, s2):
    """The same branches in double with numpy.linalg.svd.  Returns (code, x3D or None, margin): margin is the smallest relative distance
    |a - b| / max(|a|, |b|) over the comparisons a < b that the pair evaluated (w == 0 and dist == 0 compare with the vector's scale)."""
    margin = [np.inf]

    def lt(a, b):
        m = max(abs(a), abs(b))
        margin[0] = min(margin[0], abs(a - b) / m if m > 0 else 0.0)
        if TRACE is not None:
            TRACE.append((float(a), float(b)))
        return a < b

    def mats(kf):
        T = np.asarray(kf["Tcw"], F64).reshape(3, 4)
        return T, T[:, :3].T, np.asarray(kf["Ow"], F64)

    def xn(kf, kp):
        return np.array([(F64(kp["x"]) - F64(kf["cx"])) * F64(kf["invfx"]), (F64(kp["y"]) - F64(kf["cy"])) * F64(kf["invfy"]), 1.0])

    def unproject(kf, Rwc, Ow, i):
        z = F64(kf["depth"][i])
        x = (F64(kf["keys"]["x"][i]) - F64(kf["cx"])) * z * F64(kf["invfx"])
        y = (F64(kf["keys"]["y"][i]) - F64(kf["cy"])) * z * F64(kf["invfy"])
        return Rwc @ np.array([x, y, z]) + Ow

    def reproj_fails(kf, T, kp, ur, stereo, X, z, sigma2):
        x, y = T[0, :3] @ X + T[0, 3], T[1, :3] @ X + T[1, 3]
        u, v = F64(kf["fx"]) * x / z + F64(kf["cx"]), F64(kf["fy"]) * y / z + F64(kf["cy"])
        e = (u - F64(kp["x"])) ** 2 + (v - F64(kp["y"])) ** 2
        if not stereo:
            return lt(5.991 * F64(sigma2), e)
        return lt(7.8 * F64(sigma2), e + (u - F64(mbf) / z - F64(ur)) ** 2)

    kp1, kp2 = kf1["keys_un"][idx1], kf2["keys_un"][idx2]
    o1, o2 = int(kp1["octave"]), int(kp2["octave"])
    ur1, ur2 = kf1["ur"][idx1], kf2["ur"][idx2]
    stereo1, stereo2 = bool(ur1 >= 0), bool(ur2 >= 0)
    (T1, Rwc1, Ow1), (T2, Rwc2, Ow2) = mats(kf1), mats(kf2)
    xn1, xn2 = xn(kf1, kp1), xn(kf2, kp2)
    ray1, ray2 = Rwc1 @ xn1, Rwc2 @ xn2
    cos_rays = ray1 @ ray2 / (np.linalg.norm(ray1) * np.linalg.norm(ray2))
    cos1 = cos2 = cos_rays + 1
    if stereo1:
        cos1 = F64(kf1["cos"][idx1])
    elif stereo2:
        cos2 = F64(kf2["cos"][idx2])
    cos_stereo = min(cos1, cos2)
    if lt(cos_rays, cos_stereo) and lt(0.0, cos_rays) and (stereo1 or stereo2 or lt(cos_rays, 0.9998)):
        A = np.stack([xn1[0] * T1[2] - T1[0], xn1[1] * T1[2] - T1[1], xn2[0] * T2[2] - T2[0], xn2[1] * T2[2] - T2[1]])
        v = np.linalg.svd(A)[2][3]
        margin[0] = min(margin[0], abs(v[3]))
        if v[3] == 0:
            return W_ZERO, None, margin[0]
        X, code = v[:3] / v[3], TRIANGULATED
    elif stereo1 and lt(cos1, cos2):
        X, code = unproject(kf1, Rwc1, Ow1, idx1), STEREO1
    elif stereo2 and lt(cos2, cos1):
        X, code = unproject(kf2, Rwc2, Ow2, idx2), STEREO2
    else:
        return LOW_PARALLAX, None, margin[0]
    z1 = T1[2, :3] @ X + T1[2, 3]
    if not lt(0.0, z1):
        return Z1, None, margin[0]
    z2 = T2[2, :3] @ X + T2[2, 3]
    if not lt(0.0, z2):
        return Z2, None, margin[0]
    if reproj_fails(kf1, T1, kp1, ur1, stereo1, X, z1, s2[o1]):
        return REPROJ1, None, margin[0]
    if reproj_fails(kf2, T2, kp2, ur2, stereo2, X, z2, s2[o2]):
        return REPROJ2, None, margin[0]
    dist1, dist2 = np.linalg.norm(X - Ow1), np.linalg.norm(X - Ow2)
    scale = max(np.linalg.norm(X), 1.0)
    margin[0] = min(margin[0], dist1 / scale, dist2 / scale)
    if dist1 == 0 or dist2 == 0:
        return ZERO_DIST, None, margin[0]
    ratio_dist, ratio_octave = dist2 / dist1, F64(sf[o1]) / F64(sf[o2])
    if lt(ratio_dist * F64(ratio_factor), ratio_octave) or lt(ratio_octave * F64(ratio_factor), ratio_dist):
        return SCALE, None, margin[0]
    return code, X, margin[0]
