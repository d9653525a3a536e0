// Initializer.h -- Initializer::FindHomography and Initializer::FindFundamental (reference src/Initializer.cc:123-467, with Normalize,
// :748-794) restated on the flat arrays of orbfe_enqueue_find_homography_fundamental (include/orbfe.h), in plain C++ on the host: the same
// arguments, but every pointer is a HOST pointer.  Header-only, no library, no OpenCV and no device needed.  It is
//   - the form for callers without a device (and what orbfe_find_homography_fundamental uses for Normalize),
//   - written literally -- the reference's loops, the SVDs as the Jacobi of the contract with its loops rolled -- so that it is a second
//     formulation next to the kernel's wave-wide one, and
//   - the host leg of tools/bench_matchers.py --initializer.
// Compile with -ffp-contract=off: every float operation below is rounded once (contract Q4), as in the kernel.
// Not here: drawing mvSets (an input), the RH test, ReconstructH / ReconstructF / CheckRT / DecomposeE.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <utility>

#include "../../include/orbfe.h"

namespace ORB_SLAM2
{

enum { kInitializerAStride = 16, kInitializerVStride = 9 };

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

// The one-sided (Hestenes) Jacobi of cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) for an m x n float A, m >= n, held transposed:
// At[i * 16 + k] = A[k][i] (i < n <= 9, k < m <= 16), Vt[i * 9 + k].  On return W holds the singular values in descending order (strict
// selection sort) and the rows of At (the rotated columns, NOT normalised) and of Vt are carried with them.
inline void InitializerJacobi(float *At, float *Vt, double *W, int n, int m)
{
    const int as = kInitializerAStride, vs = kInitializerVStride;
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) sd += (double)At[i * as + k] * At[i * as + k];
        W[i] = sd;
        for (int k = 0; k < n; k++) Vt[i * vs + k] = i == k ? 1.f : 0.f;
    }
    const double eps = (double)FLT_EPSILON * 2;
    for (int iter = 0; iter < 30; iter++) {
        bool changed = false;
        for (int i = 0; i < n - 1; i++)
            for (int j = i + 1; j < n; j++) {
                float *Ai = At + i * as, *Aj = At + j * as;
                double a = W[i], b = W[j], p = 0;
                for (int k = 0; k < m; k++) p += (double)Ai[k] * Aj[k];
                if (std::fabs(p) <= eps * std::sqrt(a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = std::sqrt(p * p + beta * beta); // not hypot
                float c, s;
                if (beta < 0) {
                    s = (float)std::sqrt(((gamma - beta) * 0.5) / gamma);
                    c = (float)(p / (gamma * s * 2));
                } else {
                    c = (float)std::sqrt((gamma + beta) / (gamma * 2));
                    s = (float)(p / (gamma * c * 2));
                }
                a = b = 0;
                for (int k = 0; k < m; k++) {
                    const float t0 = c * Ai[k] + s * Aj[k];
                    const float t1 = -s * Ai[k] + c * Aj[k];
                    Ai[k] = t0; Aj[k] = t1;
                    a += (double)t0 * t0; b += (double)t1 * t1;
                }
                W[i] = a; W[j] = b;
                changed = true;
                float *Vi = Vt + i * vs, *Vj = Vt + j * vs;
                for (int k = 0; k < n; k++) {
                    const float t0 = c * Vi[k] + s * Vj[k];
                    const float t1 = -s * Vi[k] + c * Vj[k];
                    Vi[k] = t0; Vj[k] = t1;
                }
            }
        if (!changed) break;
    }
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) sd += (double)At[i * as + k] * At[i * as + k];
        W[i] = std::sqrt(sd);
    }
    for (int i = 0; i < n - 1; i++) {
        int j = i;
        for (int k = i + 1; k < n; k++)
            if (W[j] < W[k]) j = k;
        if (i != j) {
            std::swap(W[i], W[j]);
            for (int k = 0; k < m; k++) std::swap(At[i * as + k], At[j * as + k]);
            for (int k = 0; k < n; k++) std::swap(Vt[i * vs + k], Vt[j * vs + k]);
        }
    }
}

// a 3x3 cv::Mat product: per element a double sum over k in index order, rounded once
inline void InitializerMul3(const float a[9], const float b[9], float out[9])
{
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            double s = 0;
            for (int k = 0; k < 3; k++) s += (double)a[3 * r + k] * b[3 * k + c];
            out[3 * r + c] = (float)s;
        }
}

// cv::Mat::inv() of a 3x3 float matrix (DECOMP_LU takes the closed form): determinant and cofactors in double, det == 0 gives zeros
inline void InitializerInv3(const float m[9], float out[9])
{
    const double m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5], m20 = m[6], m21 = m[7], m22 = m[8];
    double d = m00 * (m11 * m22 - m12 * m21) - m01 * (m10 * m22 - m12 * m20) + m02 * (m10 * m21 - m11 * m20);
    if (d == 0) {
        for (int k = 0; k < 9; k++) out[k] = 0.f;
        return;
    }
    d = 1. / d;
    out[0] = (float)((m11 * m22 - m12 * m21) * d); out[1] = (float)((m02 * m21 - m01 * m22) * d); out[2] = (float)((m01 * m12 - m02 * m11) * d);
    out[3] = (float)((m12 * m20 - m10 * m22) * d); out[4] = (float)((m00 * m22 - m02 * m20) * d); out[5] = (float)((m02 * m10 - m00 * m12) * d);
    out[6] = (float)((m10 * m21 - m11 * m20) * d); out[7] = (float)((m01 * m20 - m00 * m21) * d); out[8] = (float)((m00 * m11 - m01 * m10) * d);
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
    float At[9 * kInitializerAStride], Vt[9 * kInitializerVStride];
    double W[9];
    const int as = kInitializerAStride;
    for (int i = 0; i < 8; i++) {
        const float u1 = p1[i][0], v1 = p1[i][1], u2 = p2[i][0], v2 = p2[i][1];
        const float r0[9] = {0.f, 0.f, 0.f, -u1, -v1, -1.f, v2 * u1, v2 * v1, v2};
        const float r1[9] = {u1, v1, 1.f, 0.f, 0.f, 0.f, -u2 * u1, -u2 * v1, -u2};
        for (int c = 0; c < 9; c++) { At[c * as + 2 * i] = r0[c]; At[c * as + 2 * i + 1] = r1[c]; }
    }
    InitializerJacobi(At, Vt, W, 9, 16);
    for (int k = 0; k < 9; k++) Hn[k] = Vt[8 * kInitializerVStride + k];
}

// ComputeF21 (:267-302): vt.row(8) of the 8 x 9 matrix padded with a zero ninth row, then the rank-2 step
inline void InitializerComputeF21(const float p1[8][2], const float p2[8][2], float Fn[9])
{
    float At[9 * kInitializerAStride], Vt[9 * kInitializerVStride];
    double W[9];
    const int as = kInitializerAStride, vs = kInitializerVStride;
    for (int i = 0; i < 8; i++) {
        const float u1 = p1[i][0], v1 = p1[i][1], u2 = p2[i][0], v2 = p2[i][1];
        const float r[9] = {u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1.f};
        for (int c = 0; c < 9; c++) At[c * as + i] = r[c];
    }
    for (int c = 0; c < 9; c++) At[c * as + 8] = 0.f;
    InitializerJacobi(At, Vt, W, 9, 9);
    float Fpre[9];
    for (int k = 0; k < 9; k++) Fpre[k] = Vt[8 * vs + k];
    for (int i = 0; i < 3; i++)
        for (int k = 0; k < 3; k++) At[i * as + k] = Fpre[3 * k + i];
    InitializerJacobi(At, Vt, W, 3, 3);
    float u[9], d[9], vt[9], ud[9];
    for (int i = 0; i < 3; i++) {
        const float s = W[i] > (double)FLT_MIN ? (float)(1 / W[i]) : 0.f; // the basis completion of a zero singular value is not restated
        for (int k = 0; k < 3; k++) u[3 * k + i] = At[i * as + k] * s;
    }
    for (int k = 0; k < 9; k++) { d[k] = 0.f; vt[k] = Vt[(k / 3) * vs + k % 3]; }
    d[0] = (float)W[0]; d[4] = (float)W[1]; // w.at<float>(2) = 0
    InitializerMul3(u, d, ud);
    InitializerMul3(ud, vt, Fn);
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

// a NaN score is stored with one bit pattern everywhere
inline float InitializerStoredScore(float s)
{
    if (s != s) { const uint32_t q = 0x7fc00000u; std::memcpy(&s, &q, 4); }
    return s;
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
    InitializerInv3(T2, T2inv);
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
                InitializerMul3(T2inv, Hn, t);
                InitializerMul3(t, T1, mat[0]);
                InitializerInv3(mat[0], mat[0] + 9);
            }
            if (models & 2) {
                InitializerComputeF21(p1, p2, Fn);
                InitializerMul3(T2t, Fn, t);
                InitializerMul3(t, T1, mat[1]);
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
            if (all_scores) all_scores[(size_t)model * iterations + it] = InitializerStoredScore(sc[model]);
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

} // namespace ORB_SLAM2
