// Triangulate.h -- the triangulation stage of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:286-450, with
// KeyFrame::UnprojectStereo, src/KeyFrame.cc:609-625) restated on the flat arrays of orbfe_enqueue_triangulate_pairs (include/orbfe.h),
// in plain C++ on the host: the same arguments, but every pointer (those inside the orbfe_newpoint_keyframe records too) is a HOST
// pointer and the level tables are passed in.  Header-only, no library, no OpenCV and no device needed.  It is
//   - the form for callers without a device store (the synchronous counterpart of the enqueue call),
//   - written literally -- the reference's loop with its `continue`s, the SVD as the Jacobi of the contract with its loops rolled --
//     so that it is a second formulation next to the kernel's unrolled one, and
//   - the host leg of tools/bench_matchers.py --create-new-map-points.
// Compile with -ffp-contract=off: every float operation below is rounded once (contract Q4), as in the kernel.
#pragma once

#include <cmath>
#include <cstdint>
#include <initializer_list>

#include "../../include/orbfe.h"
#include "CvMat.h"

namespace ORB_SLAM2
{

// Rwc * x (+ Ow): the product rule of MatMul, its loop kept here because Rwc is read out of Tcw transposed (Rwc[i][k] = Tcw[k][i],
// row stride 4), which MatMul's dense row-major operands do not express
inline void TriangulateRwcTimes(const float *Tcw, const float x[3], const float *plus, float out[3])
{
    for (int i = 0; i < 3; i++) {
        double s = 0;
        for (int k = 0; k < 3; k++) s += (double)Tcw[4 * k + i] * x[k];
        if (plus) s += (double)plus[i];
        out[i] = (float)s;
    }
}

// Rcw.row(r).dot(x3Dt) + tcw.at<float>(r)
inline float TriangulateRowDotPlus(const float *Tcw, int r, const float X[3])
{
    float out;
    MatMul(Tcw + 4 * r, X, 1, 3, 1, &out, nullptr, Tcw + 4 * r + 3);
    return out;
}

// KeyFrame::UnprojectStereo(i), z > 0 checked by the caller
inline void TriangulateUnprojectStereo(const orbfe_newpoint_keyframe &kf, int i, float X[3])
{
    const float z = kf.depth[i];
    const float u = kf.keys[i].x, v = kf.keys[i].y;
    const float x3Dc[3] = {(u - kf.cx) * z * kf.invfx, (v - kf.cy) * z * kf.invfy, z};
    TriangulateRwcTimes(kf.Tcw, x3Dc, kf.Ow, X);
}

// the chi-square test of :362-387 / :389-413; mbf is the CURRENT keyframe's for both
inline bool TriangulateReprojectionFails(const orbfe_newpoint_keyframe &kf, const orbfe_keypoint &kp, float kp_ur, bool bStereo, const float X[3], float z,
                                         float mbf, float sigmaSquare)
{
    const float x = TriangulateRowDotPlus(kf.Tcw, 0, X);
    const float y = TriangulateRowDotPlus(kf.Tcw, 1, X);
    const float invz = (float)(1.0 / z);
    const float u = kf.fx * x * invz + kf.cx;
    const float v = kf.fy * y * invz + kf.cy;
    const float errX = u - kp.x, errY = v - kp.y;
    if (!bStereo) return (errX * errX + errY * errY) > 5.991 * sigmaSquare;
    const float u_r = u - mbf * invz;
    const float errX_r = u_r - kp_ur;
    return (errX * errX + errY * errY + errX_r * errX_r) > 7.8 * sigmaSquare;
}

// One matched pair: the code of include/orbfe.h (a point is created iff it is <= 2) and, for a created pair, its position.
inline int TriangulatePair(const orbfe_newpoint_keyframe &kf1, const orbfe_newpoint_keyframe &kf2, int idx1, int idx2, float mbf, float ratioFactor,
                           const float *scale, const float *sigma2, int nlevels, float x3D[3])
{
    if (idx1 < 0 || idx1 >= kf1.n || idx2 < 0 || idx2 >= kf2.n) return 11;
    const orbfe_keypoint &kp1 = kf1.keys_un[idx1], &kp2 = kf2.keys_un[idx2];
    if (kp1.octave < 0 || kp1.octave >= nlevels || kp2.octave < 0 || kp2.octave >= nlevels) return 11;
    const float kp1_ur = kf1.u_right[idx1], kp2_ur = kf2.u_right[idx2];
    const bool bStereo1 = kp1_ur >= 0, bStereo2 = kp2_ur >= 0;
    if ((bStereo1 && !(kf1.depth[idx1] > 0)) || (bStereo2 && !(kf2.depth[idx2] > 0))) return 11; // UnprojectStereo would return an empty Mat

    // Check parallax between rays
    const float xn1[3] = {(kp1.x - kf1.cx) * kf1.invfx, (kp1.y - kf1.cy) * kf1.invfy, 1.f};
    const float xn2[3] = {(kp2.x - kf2.cx) * kf2.invfx, (kp2.y - kf2.cy) * kf2.invfy, 1.f};
    float ray1[3], ray2[3];
    TriangulateRwcTimes(kf1.Tcw, xn1, nullptr, ray1);
    TriangulateRwcTimes(kf2.Tcw, xn2, nullptr, ray2);
    double dot = 0;
    for (int k = 0; k < 3; k++) dot += (double)ray1[k] * ray2[k];
    const float cosParallaxRays = (float)(dot / (Norm3(ray1) * Norm3(ray2)));

    float cosParallaxStereo = cosParallaxRays + 1;
    float cosParallaxStereo1 = cosParallaxStereo;
    float cosParallaxStereo2 = cosParallaxStereo;
    if (bStereo1) cosParallaxStereo1 = kf1.cos_stereo[idx1];
    else if (bStereo2) cosParallaxStereo2 = kf2.cos_stereo[idx2];
    cosParallaxStereo = cosParallaxStereo2 < cosParallaxStereo1 ? cosParallaxStereo2 : cosParallaxStereo1; // std::min

    int code;
    if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && (bStereo1 || bStereo2 || cosParallaxRays < 0.9998)) {
        // Linear Triangulation Method
        float At[4 * kCvMatAStride], Vt[4 * kCvMatVStride];
        double W[4];
        for (int c = 0; c < 4; c++) {
            At[c * kCvMatAStride + 0] = xn1[0] * kf1.Tcw[8 + c] - kf1.Tcw[c];
            At[c * kCvMatAStride + 1] = xn1[1] * kf1.Tcw[8 + c] - kf1.Tcw[4 + c];
            At[c * kCvMatAStride + 2] = xn2[0] * kf2.Tcw[8 + c] - kf2.Tcw[c];
            At[c * kCvMatAStride + 3] = xn2[1] * kf2.Tcw[8 + c] - kf2.Tcw[4 + c];
        }
        Jacobi(At, Vt, W, 4, 4);
        const float *v = Vt + 3 * kCvMatVStride; // vt.row(3)
        if (v[3] == 0) return 4;
        // Euclidean coordinates: Mat / float is a scale
        const float alpha = (float)(1.0 / v[3]);
        for (int k = 0; k < 3; k++) x3D[k] = v[k] * alpha;
        code = 0;
    } else if (bStereo1 && cosParallaxStereo1 < cosParallaxStereo2) {
        TriangulateUnprojectStereo(kf1, idx1, x3D);
        code = 1;
    } else if (bStereo2 && cosParallaxStereo2 < cosParallaxStereo1) {
        TriangulateUnprojectStereo(kf2, idx2, x3D);
        code = 2;
    } else
        return 3; // No stereo and very low parallax

    // Check triangulation in front of cameras
    const float z1 = TriangulateRowDotPlus(kf1.Tcw, 2, x3D);
    if (z1 <= 0) return 5;
    const float z2 = TriangulateRowDotPlus(kf2.Tcw, 2, x3D);
    if (z2 <= 0) return 6;

    // Check reprojection error in first keyframe, then in the second
    if (TriangulateReprojectionFails(kf1, kp1, kp1_ur, bStereo1, x3D, z1, mbf, sigma2[kp1.octave])) return 7;
    if (TriangulateReprojectionFails(kf2, kp2, kp2_ur, bStereo2, x3D, z2, mbf, sigma2[kp2.octave])) return 8;

    // Check scale consistency
    const float normal1[3] = {x3D[0] - kf1.Ow[0], x3D[1] - kf1.Ow[1], x3D[2] - kf1.Ow[2]};
    const float dist1 = (float)Norm3(normal1);
    const float normal2[3] = {x3D[0] - kf2.Ow[0], x3D[1] - kf2.Ow[1], x3D[2] - kf2.Ow[2]};
    const float dist2 = (float)Norm3(normal2);
    if (dist1 == 0 || dist2 == 0) return 9;
    const float ratioDist = dist2 / dist1;
    const float ratioOctave = scale[kp1.octave] / scale[kp2.octave];
    if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) return 10;
    return code;
}

// Returns what the device reports in d_status (0, ORBFE_ERR_INVALID for a count outside [0, max_pairs] -- then nothing else is written --
// for a faulty pair or a negative *rows_used, ORBFE_ERR_CAPACITY for a table too small), or ORBFE_ERR_INVALID for refused arguments.
inline int TriangulatePairs(const orbfe_newpoint_keyframe *kf1, const orbfe_newpoint_keyframe *kf2, float mbf, float ratio_factor, const int32_t *pairs,
                            const int32_t *npairs, int max_pairs, const float *scale, const float *sigma2, int nlevels, uint8_t *code, float *x3d,
                            int32_t *new_points, int32_t *nnew, float *pos, int n_rows, int32_t *rows_used, int patch_has_mp)
{
    if (!kf1 || !kf2 || !pairs || !npairs || !code || !x3d || !new_points || !nnew || !scale || !sigma2 || nlevels < 1) return ORBFE_ERR_INVALID;
    if (kf1->n < 0 || kf2->n < 0 || max_pairs < 0 || max_pairs > 65535 || n_rows < 0 || (pos && !rows_used)) return ORBFE_ERR_INVALID;
    if (max_pairs > 0)
        for (const orbfe_newpoint_keyframe *kf : {kf1, kf2})
            if (!kf->keys_un || !kf->keys || !kf->u_right || !kf->depth || !kf->cos_stereo || !kf->has_mp) return ORBFE_ERR_INVALID;
    if (max_pairs == 0) { *nnew = 0; return 0; }
    const int count = *npairs;
    if (count < 0 || count > max_pairs) return ORBFE_ERR_INVALID;
    int status = 0, created = 0;
    for (int ikp = 0; ikp < count; ikp++) {
        float X[3];
        const int c = TriangulatePair(*kf1, *kf2, pairs[2 * ikp], pairs[2 * ikp + 1], mbf, ratio_factor, scale, sigma2, nlevels, X);
        code[ikp] = (uint8_t)c;
        if (c == 11) status = ORBFE_ERR_INVALID;
        if (c <= 2) {
            for (int k = 0; k < 3; k++) x3d[3 * (size_t)ikp + k] = X[k];
            created++;
        }
    }
    bool table = pos != nullptr, fits = true;
    if (table && *rows_used < 0) { status = ORBFE_ERR_INVALID; table = fits = false; }
    else if (table && (long long)*rows_used + created > n_rows) { status = ORBFE_ERR_CAPACITY; table = fits = false; }
    int k = 0;
    for (int ikp = 0; ikp < count; ikp++) {
        if (code[ikp] > 2) continue;
        const int idx1 = pairs[2 * ikp], idx2 = pairs[2 * ikp + 1];
        const int row = table ? *rows_used + k : -1;
        new_points[3 * (size_t)k] = idx1; new_points[3 * (size_t)k + 1] = idx2; new_points[3 * (size_t)k + 2] = row;
        if (table)
            for (int c = 0; c < 3; c++) pos[3 * (size_t)row + c] = x3d[3 * (size_t)ikp + c];
        if (patch_has_mp && fits) { kf1->has_mp[idx1] = 1; kf2->has_mp[idx2] = 1; } // AddMapPoint (:439-440)
        k++;
    }
    *nnew = created;
    if (table) *rows_used += created;
    return status;
}

} // namespace ORB_SLAM2
