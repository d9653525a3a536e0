// Initializer.h -- Initializer::FindHomography and Initializer::FindFundamental (reference src/Initializer.cc:123-467, with Normalize,
// :748-794) restated on the flat arrays of orbfe_enqueue_find_homography_fundamental (include/orbfe.h), in plain C++ on the host: the same
// arguments, but every pointer is a HOST pointer.  Header-only, no library, no OpenCV and no device needed.  It is
//   - the form for callers without a device (and what orbfe_find_homography_fundamental uses for Normalize),
//   - written literally -- the reference's loops, the SVDs as the Jacobi of the contract with its loops rolled -- so that it is a second
//     formulation next to the kernel's wave-wide one, and
//   - the host leg of tools/bench_matchers.py --initializer.
// Compile with -ffp-contract=off: every float operation below is rounded once (contract Q4), as in the kernel.
// Below them, ReconstructInitial is ReconstructF / ReconstructH / DecomposeE / CheckRT / Triangulate (:469-746, :797-928) with the RH test
// (:111-117) on the arrays of orbfe_enqueue_reconstruct_initial, and ReconstructAccept the parallax comparison that stays on the host.
// Not here: drawing mvSets (an input).
#pragma once

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/orbfe.h"
#include "CvMat.h"

namespace ORB_SLAM2
{

// Initializer::Normalize (:748-794) of one frame's keypoints: out = (meanX, meanY, sX, sY).  Sequential float sums in keypoint order.
inline void NormalizeKeys(const orbfe_keypoint *keys, int n, float out[4])
{
    float meanX = 0, meanY = 0;
    for (int i = 0; i < n; i++) { meanX += keys[i].x; meanY += keys[i].y; }
    meanX = meanX / n; meanY = meanY / n;
    float meanDevX = 0, meanDevY = 0;
    for (int i = 0; i < n; i++) { meanDevX += std::fabs(keys[i].x - meanX); meanDevY += std::fabs(keys[i].y - meanY); }
    meanDevX = meanDevX / n; meanDevY = meanDevY / n;
    out[0] = meanX; out[1] = meanY;
    out[2] = (float)(1.0 / meanDevX); out[3] = (float)(1.0 / meanDevY);
}

// T of Normalize (:789-793)
inline void InitializerT(const float norm[4], float T[9])
{
    for (int k = 0; k < 9; k++) T[k] = 0.f;
    T[0] = norm[2]; T[4] = norm[3]; T[8] = 1.f;
    T[2] = -norm[0] * norm[2]; T[5] = -norm[1] * norm[3];
}

// ComputeH21 (:225-265): vt.row(8) of the 16 x 9 DLT matrix
inline void InitializerComputeH21(const float p1[8][2], const float p2[8][2], float Hn[9])
{
    float At[9 * kCvMatAStride], Vt[9 * kCvMatVStride];
    double W[9];
    const int as = kCvMatAStride;
    for (int i = 0; i < 8; i++) {
        const float u1 = p1[i][0], v1 = p1[i][1], u2 = p2[i][0], v2 = p2[i][1];
        const float r0[9] = {0.f, 0.f, 0.f, -u1, -v1, -1.f, v2 * u1, v2 * v1, v2};
        const float r1[9] = {u1, v1, 1.f, 0.f, 0.f, 0.f, -u2 * u1, -u2 * v1, -u2};
        for (int c = 0; c < 9; c++) { At[c * as + 2 * i] = r0[c]; At[c * as + 2 * i + 1] = r1[c]; }
    }
    Jacobi(At, Vt, W, 9, 16);
    for (int k = 0; k < 9; k++) Hn[k] = Vt[8 * kCvMatVStride + k];
}

// ComputeF21 (:267-302): vt.row(8) of the 8 x 9 matrix padded with a zero ninth row, then the rank-2 step
inline void InitializerComputeF21(const float p1[8][2], const float p2[8][2], float Fn[9])
{
    float At[9 * kCvMatAStride], Vt[9 * kCvMatVStride];
    double W[9];
    const int as = kCvMatAStride;
    for (int i = 0; i < 8; i++) {
        const float u1 = p1[i][0], v1 = p1[i][1], u2 = p2[i][0], v2 = p2[i][1];
        const float r[9] = {u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1.f};
        for (int c = 0; c < 9; c++) At[c * as + i] = r[c];
    }
    for (int c = 0; c < 9; c++) At[c * as + 8] = 0.f;
    Jacobi(At, Vt, W, 9, 9);
    float u[9], w[3], vt[9], d[9] = {0.f}, ud[9];
    Svd3(Vt + 8 * kCvMatVStride, u, w, vt); // Fpre = vt.row(8).reshape(0, 3)
    d[0] = w[0]; d[4] = w[1];               // w.at<float>(2) = 0
    MatMul(u, d, 3, 3, 3, ud);
    MatMul(ud, vt, 3, 3, 3, Fn);
}

// the two terms of match (u1, v1, u2, v2) in CheckHomography (:336-384): returns bIn; score is the running float sum
inline bool InitializerScoreH(const float H21[9], const float H12[9], float u1, float v1, float u2, float v2, float invSigmaSquare, float &score)
{
    const float th = 5.991f;
    bool bIn = true;
    const float w2in1inv = (float)(1.0 / (H12[6] * u2 + H12[7] * v2 + H12[8]));
    const float u2in1 = (H12[0] * u2 + H12[1] * v2 + H12[2]) * w2in1inv;
    const float v2in1 = (H12[3] * u2 + H12[4] * v2 + H12[5]) * w2in1inv;
    const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) bIn = false;
    else score += th - chiSquare1;
    const float w1in2inv = (float)(1.0 / (H21[6] * u1 + H21[7] * v1 + H21[8]));
    const float u1in2 = (H21[0] * u1 + H21[1] * v1 + H21[2]) * w1in2inv;
    const float v1in2 = (H21[3] * u1 + H21[4] * v1 + H21[5]) * w1in2inv;
    const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) bIn = false;
    else score += th - chiSquare2;
    return bIn;
}

// the same of CheckFundamental (:412-464)
inline bool InitializerScoreF(const float F21[9], float u1, float v1, float u2, float v2, float invSigmaSquare, float &score)
{
    const float th = 3.841f, thScore = 5.991f;
    bool bIn = true;
    const float a2 = F21[0] * u1 + F21[1] * v1 + F21[2];
    const float b2 = F21[3] * u1 + F21[4] * v1 + F21[5];
    const float c2 = F21[6] * u1 + F21[7] * v1 + F21[8];
    const float num2 = a2 * u2 + b2 * v2 + c2;
    const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) bIn = false;
    else score += thScore - chiSquare1;
    const float a1 = F21[0] * u2 + F21[3] * v2 + F21[6];
    const float b1 = F21[1] * u2 + F21[4] * v2 + F21[7];
    const float c1 = F21[2] * u2 + F21[5] * v2 + F21[8];
    const float num1 = a1 * u1 + b1 * v1 + c1;
    const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) bIn = false;
    else score += thScore - chiSquare2;
    return bIn;
}

// Returns what the device reports in d_status (0, or ORBFE_ERR_INVALID for a pair or set index out of range), or ORBFE_ERR_INVALID for
// refused arguments (then nothing is written).  H21, F21 [9], score, best [2] (H, F); inliers_h / inliers_f [N], ninliers [2] and
// all_scores [2][iterations] may be NULL.  models: bit 0 = H, bit 1 = F; the outputs of a model that is left out stay untouched (the
// reference runs the two on a thread each, :103-104: two calls with models = 1 and models = 2 on the same arrays are that split).
inline int FindHomographyFundamental(const orbfe_keypoint *keys1, int n1, const orbfe_keypoint *keys2, int n2, const int32_t *pairs, int N,
                                     const int32_t *sets, int iterations, const float norm1[4], const float norm2[4], float sigma, float *H21, float *F21,
                                     float *score, int32_t *best, uint8_t *inliers_h, uint8_t *inliers_f, int32_t *ninliers, float *all_scores, int models = 3)
{
    if (!keys1 || !keys2 || !pairs || !sets || !norm1 || !norm2 || !H21 || !F21 || !score || !best) return ORBFE_ERR_INVALID;
    if (N < 8 || N > ORBFE_INITIALIZER_MAX_MATCHES || iterations < 1 || iterations > ORBFE_INITIALIZER_MAX_ITERATIONS || n1 < 0 || n2 < 0 ||
        n1 > ORBFE_INITIALIZER_MAX_KEYS || n2 > ORBFE_INITIALIZER_MAX_KEYS || !(sigma > 0))
        return ORBFE_ERR_INVALID;
    int status = 0;
    float T1[9], T2[9], T2inv[9], T2t[9];
    InitializerT(norm1, T1);
    InitializerT(norm2, T2);
    Inv3(T2, T2inv);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) T2t[3 * r + c] = T2[3 * c + r];
    const float invSigmaSquare = (float)(1.0 / (sigma * sigma));
    auto pair_ok = [&](int i) { return pairs[2 * i] >= 0 && pairs[2 * i] < n1 && pairs[2 * i + 1] >= 0 && pairs[2 * i + 1] < n2; };
    for (int i = 0; i < N; i++)
        if (!pair_ok(i)) status = ORBFE_ERR_INVALID;

    float best_score[2] = {0.f, 0.f};
    int best_it[2] = {-1, -1};
    float best_mat[2][18];
    for (int it = 0; it < iterations; it++) {
        // Select a minimum set
        bool ok = true;
        float p1[8][2], p2[8][2];
        for (int j = 0; j < 8 && ok; j++) {
            const int idx = sets[8 * it + j];
            if (idx < 0 || idx >= N || !pair_ok(idx)) { ok = false; break; }
            const orbfe_keypoint &k1 = keys1[pairs[2 * idx]], &k2 = keys2[pairs[2 * idx + 1]];
            p1[j][0] = (k1.x - norm1[0]) * norm1[2]; p1[j][1] = (k1.y - norm1[1]) * norm1[3];
            p2[j][0] = (k2.x - norm2[0]) * norm2[2]; p2[j][1] = (k2.y - norm2[1]) * norm2[3];
        }
        float sc[2] = {0.f, 0.f}, mat[2][18];
        if (!ok) status = ORBFE_ERR_INVALID; // a faulty hypothesis is skipped: score 0, never wins
        else {
            float Hn[9], Fn[9], t[9];
            if (models & 1) {
                InitializerComputeH21(p1, p2, Hn);
                MatMul(T2inv, Hn, 3, 3, 3, t);
                MatMul(t, T1, 3, 3, 3, mat[0]);
                Inv3(mat[0], mat[0] + 9);
            }
            if (models & 2) {
                InitializerComputeF21(p1, p2, Fn);
                MatMul(T2t, Fn, 3, 3, 3, t);
                MatMul(t, T1, 3, 3, 3, mat[1]);
            }
            for (int i = 0; i < N; i++) {
                if (!pair_ok(i)) continue; // a faulty match adds nothing
                const orbfe_keypoint &k1 = keys1[pairs[2 * i]], &k2 = keys2[pairs[2 * i + 1]];
                if (models & 1) InitializerScoreH(mat[0], mat[0] + 9, k1.x, k1.y, k2.x, k2.y, invSigmaSquare, sc[0]);
                if (models & 2) InitializerScoreF(mat[1], k1.x, k1.y, k2.x, k2.y, invSigmaSquare, sc[1]);
            }
        }
        for (int model = 0; model < 2; model++) {
            if (!(models >> model & 1)) continue;
            if (all_scores) all_scores[(size_t)model * iterations + it] = Stored(sc[model]);
            if (sc[model] > best_score[model]) {
                best_score[model] = sc[model]; best_it[model] = it;
                std::memcpy(best_mat[model], mat[model], sizeof(mat[model]));
            }
        }
    }
    for (int model = 0; model < 2; model++) {
        if (!(models >> model & 1)) continue;
        uint8_t *inl = model == 0 ? inliers_h : inliers_f;
        score[model] = best_score[model]; best[model] = best_it[model];
        int count = 0;
        for (int i = 0; i < N; i++) {
            bool in = false;
            if (best_it[model] >= 0 && pair_ok(i)) {
                const orbfe_keypoint &k1 = keys1[pairs[2 * i]], &k2 = keys2[pairs[2 * i + 1]];
                float unused = 0.f;
                in = model == 0 ? InitializerScoreH(best_mat[0], best_mat[0] + 9, k1.x, k1.y, k2.x, k2.y, invSigmaSquare, unused)
                                : InitializerScoreF(best_mat[1], k1.x, k1.y, k2.x, k2.y, invSigmaSquare, unused);
            }
            if (inl) inl[i] = in ? 1 : 0;
            count += in;
        }
        if (ninliers) ninliers[model] = count;
        if (best_it[model] >= 0) std::memcpy(model == 0 ? H21 : F21, best_mat[model], 9 * sizeof(float));
    }
    return status;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// ReconstructF / ReconstructH / DecomposeE / CheckRT / Triangulate (:469-746, :797-928) on the flat arrays of
// orbfe_enqueue_reconstruct_initial (include/orbfe.h): the same arguments, every pointer a HOST pointer.

inline void ReconstructK(const float K4[4], float K[9])
{
    for (int k = 0; k < 9; k++) K[k] = 0.f;
    K[0] = K4[0]; K[4] = K4[1]; K[2] = K4[2]; K[5] = K4[3]; K[8] = 1.f;
}

// a NaN is stored with one bit pattern everywhere
inline void ReconstructStore(float *dst, const float *src, int n)
{
    for (int k = 0; k < n; k++) dst[k] = Stored(src[k]);
}

// the order of the sorted cosines: that of the floats, -0 before +0, any NaN after every number
inline uint32_t ReconstructOrderKey(float c)
{
    uint32_t b;
    std::memcpy(&b, &c, 4);
    if (c != c) return 0xFFFFFFFFu;
    return (b >> 31) ? ~b : (b | 0x80000000u);
}

inline float ReconstructKeyValue(uint32_t key)
{
    uint32_t b = (key >> 31) ? (key & 0x7FFFFFFFu) : ~key;
    if (key == 0xFFFFFFFFu) b = 0x7FC00000u;
    float c;
    std::memcpy(&c, &b, 4);
    return c;
}

// DecomposeE on E21 = K.t() * F21 * K (:478-496, :908-928): the four hypotheses (R1, t), (R2, t), (R1, -t), (R2, -t)
inline void ReconstructHypothesesF(const float F21[9], const float K[9], float vR[8][9], float vt[8][3])
{
    float Kt[9], tmp[9], E[9], u[9], w[3], vtm[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) Kt[3 * r + c] = K[3 * c + r];
    MatMul(Kt, F21, 3, 3, 3, tmp);
    MatMul(tmp, K, 3, 3, 3, E);
    Svd3(E, u, w, vtm);
    float t[3] = {u[2], u[5], u[8]};
    Unit(t);
    const float W[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1}, Wt[9] = {0, 1, 0, -1, 0, 0, 0, 0, 1};
    float R[2][9];
    for (int which = 0; which < 2; which++) {
        MatMul(u, which ? Wt : W, 3, 3, 3, tmp);
        MatMul(tmp, vtm, 3, 3, 3, R[which]);
        if (Det3(R[which]) < 0)
            for (int k = 0; k < 9; k++) R[which][k] = -R[which][k];
    }
    for (int h = 0; h < 4; h++) {
        for (int k = 0; k < 9; k++) vR[h][k] = R[h & 1][k];
        for (int k = 0; k < 3; k++) vt[h][k] = h < 2 ? t[k] : -t[k];
    }
}

// The eight hypotheses of ReconstructH (:583-685).  Returns false under the test of :596.  vn is never read and is not computed.
inline bool ReconstructHypothesesH(const float H21[9], const float K[9], float vR[8][9], float vt[8][3])
{
    float invK[9], tmp[9], A[9], U[9], w[3], Vt[9];
    Inv3(K, invK);
    MatMul(invK, H21, 3, 3, 3, tmp);
    MatMul(tmp, K, 3, 3, 3, A);
    Svd3(A, U, w, Vt);
    const float s = (float)(Det3(U) * Det3(Vt));
    const float d1 = w[0], d2 = w[1], d3 = w[2];
    if (d1 / d2 < 1.00001 || d2 / d3 < 1.00001) return false;
    const float aux1 = std::sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
    const float aux3 = std::sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
    const float x1[] = {aux1, aux1, -aux1, -aux1};
    const float x3[] = {aux3, -aux3, aux3, -aux3};
    const float aux_stheta = std::sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
    const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
    const float stheta[] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
    const float aux_sphi = std::sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
    const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
    const float sphi[] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
    const double alpha = s;
    for (int i = 0; i < 8; i++) {
        float Rp[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tp[3];
        if (i < 4) { // case d' = d2
            Rp[0] = ctheta; Rp[2] = -stheta[i]; Rp[6] = stheta[i]; Rp[8] = ctheta;
            tp[0] = x1[i]; tp[1] = 0; tp[2] = -x3[i];
            for (int k = 0; k < 3; k++) tp[k] = tp[k] * (d1 - d3);
        } else {     // case d' = -d2
            Rp[0] = cphi; Rp[2] = sphi[i - 4]; Rp[4] = -1; Rp[6] = sphi[i - 4]; Rp[8] = -cphi;
            tp[0] = x1[i - 4]; tp[1] = 0; tp[2] = x3[i - 4];
            for (int k = 0; k < 3; k++) tp[k] = tp[k] * (d1 + d3);
        }
        MatMul(U, Rp, 3, 3, 3, tmp, &alpha); // s * U * Rp: the scale is the gemm's alpha (the reading tagged in include/orbfe.h)
        MatMul(tmp, Vt, 3, 3, 3, vR[i]);
        MatMul(U, tp, 3, 3, 1, vt[i]);
        Unit(vt[i]);
    }
    return true;
}

// P2 = K * [R|t] (3x4) and O2 = -R.t() * t of CheckRT (:819-825)
inline void ReconstructCamera2(const float R[9], const float t[3], const float K[9], float P2[12], float O2[3])
{
    float Rt[12], Rtr[9];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) { Rt[4 * r + c] = R[3 * r + c]; Rtr[3 * r + c] = R[3 * c + r]; }
        Rt[4 * r + 3] = t[r];
    }
    MatMul(K, Rt, 3, 3, 4, P2);
    const double minus = -1.0;
    MatMul(Rtr, t, 3, 3, 1, O2, &minus);
}

// One iteration of CheckRT's loop (:829-893) for an inlier match: the code (1..7 of orbfe_enqueue_reconstruct_initial), its cosine and point.
inline int ReconstructCheckMatch(const float R[9], const float t[3], const float K4[4], const float P2[12], const float O2[3], float kp1x, float kp1y,
                                 float kp2x, float kp2y, float th2, float &cosParallax, float p3dC1[3])
{
    const float fx = K4[0], fy = K4[1], cx = K4[2], cy = K4[3];
    const float P1[12] = {fx, 0, cx, 0, 0, fy, cy, 0, 0, 0, 1, 0};
    // Triangulate (:733-746)
    float At[4 * kCvMatAStride], Vt[4 * kCvMatVStride];
    double W[4];
    for (int c = 0; c < 4; c++) {
        At[c * kCvMatAStride + 0] = kp1x * P1[8 + c] - P1[c];
        At[c * kCvMatAStride + 1] = kp1y * P1[8 + c] - P1[4 + c];
        At[c * kCvMatAStride + 2] = kp2x * P2[8 + c] - P2[c];
        At[c * kCvMatAStride + 3] = kp2y * P2[8 + c] - P2[4 + c];
    }
    Jacobi(At, Vt, W, 4, 4);
    const float *x3D = Vt + 3 * kCvMatVStride;
    const float a = (float)(1.0 / x3D[3]);
    for (int k = 0; k < 3; k++) p3dC1[k] = x3D[k] * a;
    cosParallax = 0.f;
    if (!std::isfinite(p3dC1[0]) || !std::isfinite(p3dC1[1]) || !std::isfinite(p3dC1[2])) return 1;
    // Check parallax
    float normal2[3];
    double dot = 0;
    for (int k = 0; k < 3; k++) {
        normal2[k] = p3dC1[k] - O2[k];
        dot += (double)p3dC1[k] * normal2[k];
    }
    const float dist1 = (float)Norm3(p3dC1), dist2 = (float)Norm3(normal2);
    cosParallax = (float)(dot / (double)(dist1 * dist2));
    // Check depth in front of first camera (only if enough parallax, as "infinite" points can easily go to negative depth)
    if (p3dC1[2] <= 0 && cosParallax < 0.99998) return 2;
    // Check depth in front of second camera
    float p3dC2[3];
    MatMul(R, p3dC1, 3, 3, 1, p3dC2, nullptr, t);
    if (p3dC2[2] <= 0 && cosParallax < 0.99998) return 3;
    // Check reprojection error in first image
    const float invZ1 = (float)(1.0 / p3dC1[2]);
    const float im1x = fx * p3dC1[0] * invZ1 + cx, im1y = fy * p3dC1[1] * invZ1 + cy;
    const float squareError1 = (im1x - kp1x) * (im1x - kp1x) + (im1y - kp1y) * (im1y - kp1y);
    if (squareError1 > th2) return 4;
    // Check reprojection error in second image
    const float invZ2 = (float)(1.0 / p3dC2[2]);
    const float im2x = fx * p3dC2[0] * invZ2 + cx, im2y = fy * p3dC2[1] * invZ2 + cy;
    const float squareError2 = (im2x - kp2x) * (im2x - kp2x) + (im2y - kp2y) * (im2y - kp2y);
    if (squareError2 > th2) return 5;
    return cosParallax < 0.99998 ? 7 : 6;
}

// The parallax test of ReconstructF (:524) / ReconstructH (:720) on the chosen hypothesis's cosine: the one comparison that stays on
// the host (acos is the platform's).  cos_parallax == 2 stands for nGood == 0, parallax = 0.
inline bool ReconstructAccept(int model, float cos_parallax, float minParallax)
{
    float parallax = 0;
    if (cos_parallax != 2.0f) parallax = (float)(std::acos(cos_parallax) * 180 / 3.1415926535897932384626433832795);
    return model == 0 ? parallax >= minParallax : parallax > minParallax;
}

// Returns what the device reports in d_status (0, or ORBFE_ERR_INVALID for a pair index out of range), or ORBFE_ERR_INVALID for refused
// arguments (then nothing is written).  codes [8][N] may be NULL; every other pointer is required.
inline int ReconstructInitial(const orbfe_keypoint *keys1, int n1, const orbfe_keypoint *keys2, int n2, const int32_t *pairs, int N, const float *H21,
                              const float *F21, const float *score, const int32_t *best, const uint8_t *inliers_h, const uint8_t *inliers_f, const float *K4,
                              float sigma, int min_triangulated, int model, int32_t *out_model, float *hyp_R, float *hyp_t, int32_t *ngood, float *cos_parallax,
                              int32_t *result, int32_t *choice, float *R21, float *t21, float *p3d, uint8_t *triangulated, uint8_t *codes)
{
    if (!keys1 || !keys2 || !pairs || !H21 || !F21 || !score || !best || !inliers_h || !inliers_f || !K4) return ORBFE_ERR_INVALID;
    if (!out_model || !hyp_R || !hyp_t || !ngood || !cos_parallax || !result || !choice || !R21 || !t21 || !p3d || !triangulated) return ORBFE_ERR_INVALID;
    if (N < 1 || N > ORBFE_INITIALIZER_MAX_MATCHES || n1 < 0 || n2 < 0 || n1 > ORBFE_INITIALIZER_MAX_KEYS || n2 > ORBFE_INITIALIZER_MAX_KEYS || !(sigma > 0) ||
        !(K4[0] > 0) || !(K4[1] > 0) || min_triangulated < 0 || model < -1 || model > 1)
        return ORBFE_ERR_INVALID;
    int status = 0;
    if (model == -1) { // :111-117
        const float SH = score[0], SF = score[1];
        const float RH = SH / (SH + SF);
        model = RH > 0.40 ? 0 : 1;
    }
    *out_model = model;
    const uint8_t *vbMatchesInliers = model == 0 ? inliers_h : inliers_f;
    auto pair_ok = [&](int i) { return pairs[2 * i] >= 0 && pairs[2 * i] < n1 && pairs[2 * i + 1] >= 0 && pairs[2 * i + 1] < n2; };
    int Ninl = 0;
    for (int i = 0; i < N; i++) {
        if (vbMatchesInliers[i]) Ninl++;
        if (!pair_ok(i)) status = ORBFE_ERR_INVALID;
    }
    for (int h = 0; h < 8; h++) { ngood[h] = 0; cos_parallax[h] = 2.0f; }
    if (codes) std::memset(codes, 0, 8 * (size_t)N);
    for (int i = 0; i < n1; i++) { p3d[3 * i] = p3d[3 * i + 1] = p3d[3 * i + 2] = 0.f; triangulated[i] = 0; }
    *choice = -1;
    if (best[model] < 0) { *result = 1; return status; }
    float K[9], vR[8][9], vt[8][3];
    ReconstructK(K4, K);
    int nhyp = 4;
    if (model == 0) {
        if (!ReconstructHypothesesH(H21, K, vR, vt)) { *result = 2; return status; }
        nhyp = 8;
    } else
        ReconstructHypothesesF(F21, K, vR, vt);
    const float th2 = (float)(4.0 * (sigma * sigma));
    std::vector<uint32_t> vCosParallax;
    for (int h = 0; h < nhyp; h++) {
        ReconstructStore(hyp_R + 9 * h, vR[h], 9);
        ReconstructStore(hyp_t + 3 * h, vt[h], 3);
        float P2[12], O2[3];
        ReconstructCamera2(vR[h], vt[h], K, P2, O2);
        vCosParallax.clear();
        int nGood = 0;
        for (int i = 0; i < N; i++) {
            if (!vbMatchesInliers[i] || !pair_ok(i)) continue;
            const orbfe_keypoint &kp1 = keys1[pairs[2 * i]], &kp2 = keys2[pairs[2 * i + 1]];
            float cosParallax, p3dC1[3];
            const int code = ReconstructCheckMatch(vR[h], vt[h], K4, P2, O2, kp1.x, kp1.y, kp2.x, kp2.y, th2, cosParallax, p3dC1);
            if (codes) codes[(size_t)h * N + i] = (uint8_t)code;
            if (code < 6) continue;
            vCosParallax.push_back(ReconstructOrderKey(cosParallax));
            nGood++;
        }
        ngood[h] = nGood;
        if (nGood > 0) {
            std::sort(vCosParallax.begin(), vCosParallax.end());
            const size_t idx = std::min(50, int(vCosParallax.size() - 1));
            cos_parallax[h] = ReconstructKeyValue(vCosParallax[idx]);
        }
    }
    int chosen = -1;
    if (model == 1) { // :498-566
        const int maxGood = std::max(ngood[0], std::max(ngood[1], std::max(ngood[2], ngood[3])));
        const int nMinGood = std::max(static_cast<int>(0.9 * Ninl), min_triangulated);
        int nsimilar = 0;
        for (int h = 0; h < 4; h++)
            if (ngood[h] > 0.7 * maxGood) nsimilar++;
        if (!(maxGood < nMinGood || nsimilar > 1))
            for (int h = 3; h >= 0; h--)
                if (ngood[h] == maxGood) chosen = h; // the else-if chain never looks past the first
    } else {          // :688-720
        int bestGood = 0, secondBestGood = 0, bestSolutionIdx = -1;
        for (int i = 0; i < 8; i++) {
            if (ngood[i] > bestGood) { secondBestGood = bestGood; bestGood = ngood[i]; bestSolutionIdx = i; }
            else if (ngood[i] > secondBestGood) secondBestGood = ngood[i];
        }
        if (secondBestGood < 0.75 * bestGood && bestGood > min_triangulated && bestGood > 0.9 * Ninl) chosen = bestSolutionIdx;
    }
    *choice = chosen;
    if (chosen < 0) { *result = 3; return status; }
    *result = 0;
    ReconstructStore(R21, vR[chosen], 9);
    ReconstructStore(t21, vt[chosen], 3);
    float P2[12], O2[3];
    ReconstructCamera2(vR[chosen], vt[chosen], K, P2, O2);
    for (int i = 0; i < N; i++) {
        if (!vbMatchesInliers[i] || !pair_ok(i)) continue;
        const orbfe_keypoint &kp1 = keys1[pairs[2 * i]], &kp2 = keys2[pairs[2 * i + 1]];
        float cosParallax, p3dC1[3];
        const int code = ReconstructCheckMatch(vR[chosen], vt[chosen], K4, P2, O2, kp1.x, kp1.y, kp2.x, kp2.y, th2, cosParallax, p3dC1);
        if (code < 6) continue;
        float *dst = p3d + 3 * (size_t)pairs[2 * i];
        dst[0] = p3dC1[0]; dst[1] = p3dC1[1]; dst[2] = p3dC1[2];
        triangulated[pairs[2 * i]] = code == 7;
    }
    return status;
}

} // namespace ORB_SLAM2
