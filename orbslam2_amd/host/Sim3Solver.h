// Sim3Solver.h -- the host side of the Sim3Solver port (reference src/Sim3Solver.cc): the iteration table and the
// draw rows that orbfe_enqueue_sim3_ransac_batch takes, the literal host form of what its kernels compute (the constructor's filter,
// ComputeSim3, CheckInliers, the events) on flat arrays, and ORB_SLAM2::Sim3Solver, which answers the reference's SetRansacParameters /
// iterate / find / GetEstimated* from the rows of either backend -- the host form below or the rows fetched from the device -- so that
// the loop of src/LoopClosing.cc:322-378 compiles as it stands.  Header-only, no OpenCV, no device needed.  Written literally, loops
// rolled: a second formulation next to the kernels' unrolled one, equal to them and to tests/sim3_solver_model.py bit for bit
// (tests/sim3_solver_mirror/mirror_main.cpp is the driver).  Compile with -ffp-contract=off, as CvMat.h asks.
//
// The keypoint read for sigmaSquare is the slot itself: that equals MapPoint::GetIndexInKeyFrame whenever a map point is observed once
// per keyframe.  The two replacements of OpenCV steps (cv::eigen -> a cyclic two-sided Jacobi in double; atan2 + cv::Rodrigues -> the
// rotation matrix of the unit quaternion) are stated in DESIGN.md section 4o.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/orbfe.h"
#include "CvMat.h"

namespace ORB_SLAM2
{

// ---------------------------------------------------------------------------------------------------------------- table and draws
// SetRansacParameters (:115-139) for N correspondences: mRansacMaxIts afterwards; 0 stands for the bNoMore exit of iterate (:147-151)
inline int Sim3RansacIterations(int N, double prob, int minInliers, int maxIts)
{
    if (N < minInliers) return 0;
    double n;
    if (minInliers == N) n = 1;
    else {
        const float epsilon = (float)minInliers / N;
        n = std::ceil(std::log(1 - prob) / std::log(1 - std::pow((double)epsilon, 3.0)));
    }
    const int nIterations = !(n < maxIts) ? maxIts : (int)n; // the clamp before the conversion: no overflow
    return std::max(1, std::min(nIterations, maxIts));
}

// d_its_for_n of orbfe_enqueue_sim3_ransac_batch: one entry per N in [0, maxPairs]
inline std::vector<int32_t> Sim3RansacIterationTable(int maxPairs, double prob, int minInliers, int maxIts)
{
    std::vector<int32_t> t((size_t)maxPairs + 1);
    for (int N = 0; N <= maxPairs; N++) t[N] = Sim3RansacIterations(N, prob, minInliers, maxIts);
    return t;
}

// a draw row [maxIts][3] of raw rand() values, as DUtils::Random::RandomInt consumes them
inline void DrawSim3Sets(uint32_t *draws, int maxIts)
{
    for (int k = 0; k < 3 * maxIts; k++) draws[k] = (uint32_t)rand();
}

// DUtils::Random::RandomInt(0, d - 1) on a raw value (Thirdparty/DLib/src/Random.cpp:47-50; RAND_MAX = 2^31 - 1)
inline int Sim3RandomInt(uint32_t r, int d) { return (int)(((double)r / 2147483648.0) * d); }

// the three correspondences of :164-178: vAvailableIndices starts as 0 .. N-1 and each draw swaps with the back and pops
inline void Sim3DrawSet(const uint32_t r[3], int N, int32_t ids[3])
{
    std::vector<int> avail(N);
    for (int i = 0; i < N; i++) avail[i] = i;
    for (int i = 0; i < 3; i++) {
        const int randi = Sim3RandomInt(r[i], (int)avail.size());
        ids[i] = avail[randi];
        avail[randi] = avail.back();
        avail.pop_back();
    }
}

// ---------------------------------------------------------------------------------------------------------------- the host form
struct Sim3Table { // per correspondence: mvX3Dc1, mvX3Dc2, mvP1im1, mvP2im2, mvnMaxError1 / 2 (as the float they are compared as)
    std::vector<float> X1, X2, p1, p2, g1, g2;
};

struct Sim3Rows { // the rows of one candidate, as the device writes them
    int32_t status = 0, n_corr = 0, n_its = 0, n_events = 0;
    int max_pairs = 0, max_its = 0, words = 0;
    std::vector<int32_t> corr, sets, events;   // [max_pairs][2], [max_its][3], [max_its]
    std::vector<orbfe_sim3_hypothesis> hyp;    // [max_its]
    std::vector<uint32_t> bits;                // [max_its][words]
};

// the rows of candidate c as fetched from the device after orbfe_enqueue_sim3_ransac_batch (host copies of its output arrays, all
// candidates).  corr / bits may be NULL when they were not downloaded: iterate() then leaves vbInliers empty of inliers.
inline Sim3Rows Sim3RowsOfCandidate(int c, int max_pairs, int max_its, const int32_t *status, const int32_t *n_corr, const int32_t *n_its,
                                    const int32_t *n_events, const int32_t *events, const orbfe_sim3_hypothesis *hyp, const int32_t *corr,
                                    const uint32_t *bits)
{
    Sim3Rows o;
    o.status = status ? status[c] : 0; o.n_corr = n_corr[c]; o.n_its = n_its[c]; o.n_events = n_events[c];
    o.max_pairs = max_pairs; o.max_its = max_its; o.words = (max_pairs + 31) / 32;
    o.events.assign(events + (size_t)c * max_its, events + (size_t)(c + 1) * max_its);
    o.hyp.assign(hyp + (size_t)c * max_its, hyp + (size_t)(c + 1) * max_its);
    if (corr) o.corr.assign(corr + (size_t)c * 2 * max_pairs, corr + (size_t)(c + 1) * 2 * max_pairs);
    else o.corr.assign((size_t)2 * max_pairs, -1);
    if (bits) o.bits.assign(bits + (size_t)c * max_its * o.words, bits + (size_t)(c + 1) * max_its * o.words);
    else o.bits.assign((size_t)max_its * o.words, 0u);
    return o;
}

inline void Sim3ToImage(const float X[3], const float cam[4], float p[2])
{
    const float invz = 1 / X[2];
    const float x = X[0] * invz, y = X[1] * invz;
    p[0] = cam[0] * x + cam[2];
    p[1] = cam[1] * y + cam[3];
}

// the constructor (:63-110) on keypoint slots.  pairs: (idx1, idx2) in ascending idx1.  Returns the status.
inline int Sim3Filter(const orbfe_keypoint *keys1, int n1, const float *T1w, const float *pos1, const int32_t *valid1, const orbfe_keypoint *keys2, int n2,
                      const float *T2w, const float *pos2, const int32_t *valid2, const int32_t *pairs, int n_pairs, const float *sigma2, int nlevels,
                      const float cam[4], std::vector<int32_t> &corr, Sim3Table &T)
{
    int status = 0;
    for (int p = 0; p < n_pairs; p++) {
        const int i1 = pairs[2 * p], i2 = pairs[2 * p + 1];
        bool ok = i1 >= 0 && i1 < n1 && i2 >= 0 && i2 < n2;
        if (ok) ok = keys1[i1].octave >= 0 && keys1[i1].octave < nlevels && keys2[i2].octave >= 0 && keys2[i2].octave < nlevels;
        if (!ok) { status = ORBFE_ERR_INVALID; continue; }
        if (!valid1[i1] || !valid2[i2]) continue;
        float X1[3], X2[3], q1[2], q2[2];
        for (int r = 0; r < 3; r++) { // Rcw * Xw + tcw row by row: the rows of [R | t] are 4 floats apart
            MatMul(T1w + 4 * r, pos1 + 3 * (size_t)i1, 1, 3, 1, &X1[r], nullptr, T1w + 4 * r + 3);
            MatMul(T2w + 4 * r, pos2 + 3 * (size_t)i2, 1, 3, 1, &X2[r], nullptr, T2w + 4 * r + 3);
        }
        Sim3ToImage(X1, cam, q1);
        Sim3ToImage(X2, cam, q2);
        corr.push_back(i1); corr.push_back(i2);
        for (int r = 0; r < 3; r++) { T.X1.push_back(X1[r]); T.X2.push_back(X2[r]); }
        for (int r = 0; r < 2; r++) { T.p1.push_back(q1[r]); T.p2.push_back(q2[r]); }
        T.g1.push_back((float)(size_t)(9.210 * (double)sigma2[keys1[i1].octave]));   // mvnMaxError is a vector<size_t>
        T.g2.push_back((float)(size_t)(9.210 * (double)sigma2[keys2[i2].octave]));
    }
    return status;
}

// the cyclic two-sided Jacobi of DESIGN.md section 4o on a symmetric 4 x 4 in double; V's columns are the eigenvectors
inline int Sim3Jacobi4(double A[4][4], double V[4][4])
{
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) V[i][j] = i == j ? 1.0 : 0.0;
    int sweeps = 0;
    for (int it = 0; it < 30; it++) {
        bool rotated = false;
        for (int p = 0; p < 3; p++)
            for (int q = p + 1; q < 4; q++) {
                const double apq = A[p][q], g = std::fabs(apq);
                if (std::fabs(A[p][p]) + g == std::fabs(A[p][p]) && std::fabs(A[q][q]) + g == std::fabs(A[q][q])) {
                    A[p][q] = A[q][p] = 0.0;
                    continue;
                }
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                double t = 1.0 / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                if (theta < 0) t = -t;
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                A[p][p] = A[p][p] - t * apq;
                A[q][q] = A[q][q] + t * apq;
                A[p][q] = A[q][p] = 0.0;
                for (int r = 0; r < 4; r++)
                    if (r != p && r != q) {
                        const double arp = A[r][p], arq = A[r][q];
                        A[r][p] = A[p][r] = c * arp - s * arq;
                        A[r][q] = A[q][r] = s * arp + c * arq;
                    }
                for (int r = 0; r < 4; r++) {
                    const double vrp = V[r][p], vrq = V[r][q];
                    V[r][p] = c * vrp - s * vrq;
                    V[r][q] = s * vrp + c * vrq;
                }
                rotated = true;
            }
        if (!rotated) break;
        sweeps++;
    }
    return sweeps;
}

struct Sim3Hypothesis { float R[9], t[3], s, sR[9], sRinv[9], tinv[3]; };

// ComputeCentroid (:216-225): cv::reduce(SUM) is a float sum in index order, `/ P.cols` a scale by (float)(1.0 / 3)
inline void Sim3Centroid(const float P[9], float Pr[9], float C[3])
{
    const float third = (float)(1.0 / 3);
    for (int r = 0; r < 3; r++) {
        C[r] = ReduceSum(P + 3 * r, 3) * third;
        for (int i = 0; i < 3; i++) Pr[3 * r + i] = P[3 * r + i] - C[r];
    }
}

// ComputeSim3 (:227-338) on P1, P2 (3 x 3 row-major, column i the i-th drawn point)
inline void Sim3Compute(const float P1[9], const float P2[9], bool fixScale, Sim3Hypothesis &h)
{
    float Pr1[9], Pr2[9], O1[3], O2[3], Pr1t[9], M[9];
    Sim3Centroid(P1, Pr1, O1);
    Sim3Centroid(P2, Pr2, O2);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) Pr1t[3 * r + c] = Pr1[3 * c + r];
    MatMul(Pr2, Pr1t, 3, 3, 3, M);
    const float m00 = M[0], m01 = M[1], m02 = M[2], m10 = M[3], m11 = M[4], m12 = M[5], m20 = M[6], m21 = M[7], m22 = M[8];
    const float N11 = m00 + m11 + m22, N12 = m12 - m21, N13 = m20 - m02, N14 = m01 - m10, N22 = m00 - m11 - m22, N23 = m01 + m10, N24 = m20 + m02,
                N33 = -m00 + m11 - m22, N34 = m12 + m21, N44 = -m00 - m11 + m22;
    double A[4][4] = {{N11, N12, N13, N14}, {N12, N22, N23, N24}, {N13, N23, N33, N34}, {N14, N24, N34, N44}}, V[4][4];
    Sim3Jacobi4(A, V);
    int top = 0;
    for (int i = 1; i < 4; i++)
        if (A[i][i] > A[top][top]) top = i; // first strict maximum
    const double w = V[0][top], x = V[1][top], y = V[2][top], z = V[3][top];
    const double ww = w * w, xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    const double n = ww + xx + yy + zz;
    const double Rd[9] = {(ww + xx - yy - zz) / n, (2.0 * (xy - wz)) / n, (2.0 * (xz + wy)) / n, (2.0 * (xy + wz)) / n, (ww - xx + yy - zz) / n,
                          (2.0 * (yz - wx)) / n, (2.0 * (xz - wy)) / n, (2.0 * (yz + wx)) / n, (ww - xx - yy + zz) / n};
    for (int k = 0; k < 9; k++) h.R[k] = (float)Rd[k];
    float P3[9];
    MatMul(h.R, Pr2, 3, 3, 3, P3);
    if (!fixScale) {
        const double nom = Dot(Pr1, P3, 9);                          // Mat::dot: a double sum
        const double den = SumOfSquaredFloats(P3, 9);                // cv::pow(., 2) is a float product, den a double sum of them
        h.s = Ratio(nom, den);
    } else
        h.s = 1.0f;
    const double ms = -(double)h.s, minus1 = -1.0;
    MatMul(h.R, O2, 3, 3, 1, h.t, &ms, O1);                         // O1 - s * R * O2: one gemm
    const float inv = (float)(1.0 / (double)h.s);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            h.sR[3 * r + c] = h.s * h.R[3 * r + c];
            h.sRinv[3 * r + c] = h.R[3 * c + r] * inv;               // (1.0 / s) * R.t(): a scale by (float)(1.0 / s)
        }
    MatMul(h.sRinv, h.t, 3, 3, 1, h.tinv, &minus1);
}

// one side of CheckInliers: |a - Project(X, A, b)|^2 (sign = +1) or |Project(X, A, b) - a|^2, the same number
inline float Sim3Error(const float X[3], const float A[9], const float b[3], const float cam[4], const float a[2])
{
    float P[3], q[2];
    MatMul(A, X, 3, 3, 1, P, nullptr, b);
    Sim3ToImage(P, cam, q);
    const float d0 = a[0] - q[0], d1 = a[1] - q[1];
    return (float)((double)d0 * d0 + (double)d1 * d1);
}

// every row of orbfe_enqueue_sim3_ransac_batch for one candidate, computed on the host
inline Sim3Rows Sim3RansacHost(const orbfe_keypoint *keys1, int n1, const float *T1w, const float *pos1, const int32_t *valid1, const orbfe_keypoint *keys2,
                               int n2, const float *T2w, const float *pos2, const int32_t *valid2, const int32_t *pairs, int n_pairs, const uint32_t *draws,
                               int max_pairs, int fix_scale, int min_inliers, int max_its, const int32_t *its_for_n, const float *sigma2, int nlevels,
                               const float cam[4])
{
    Sim3Rows o;
    o.max_pairs = max_pairs; o.max_its = max_its; o.words = (max_pairs + 31) / 32;
    o.corr.assign((size_t)2 * max_pairs, -1);
    o.sets.assign((size_t)3 * max_its, -1);
    o.events.assign(max_its, -1);
    o.hyp.assign(max_its, orbfe_sim3_hypothesis());
    o.bits.assign((size_t)max_its * o.words, 0u);
    if (n_pairs < 0 || n_pairs > max_pairs) { o.status = ORBFE_ERR_INVALID; return o; }
    std::vector<int32_t> corr;
    Sim3Table T;
    o.status = Sim3Filter(keys1, n1, T1w, pos1, valid1, keys2, n2, T2w, pos2, valid2, pairs, n_pairs, sigma2, nlevels, cam, corr, T);
    const int N = (int)corr.size() / 2;
    o.n_corr = N;
    std::memcpy(o.corr.data(), corr.data(), sizeof(int32_t) * corr.size());
    o.n_its = std::min(its_for_n[N], max_its);
    int best = 0;
    for (int k = 0; k < o.n_its; k++) {
        int32_t *ids = &o.sets[3 * (size_t)k];
        Sim3DrawSet(draws + 3 * (size_t)k, N, ids);
        float P1[9], P2[9];
        for (int i = 0; i < 3; i++)
            for (int r = 0; r < 3; r++) { P1[3 * r + i] = T.X1[3 * (size_t)ids[i] + r]; P2[3 * r + i] = T.X2[3 * (size_t)ids[i] + r]; }
        Sim3Hypothesis h;
        Sim3Compute(P1, P2, fix_scale != 0, h);
        int count = 0;
        for (int j = 0; j < N; j++) {
            const float err1 = Sim3Error(&T.X2[3 * (size_t)j], h.sR, h.t, cam, &T.p1[2 * (size_t)j]);
            const float err2 = Sim3Error(&T.X1[3 * (size_t)j], h.sRinv, h.tinv, cam, &T.p2[2 * (size_t)j]);
            if (err1 < T.g1[j] && err2 < T.g2[j]) {
                o.bits[(size_t)k * o.words + (j >> 5)] |= 1u << (j & 31);
                count++;
            }
        }
        orbfe_sim3_hypothesis &H = o.hyp[k];
        H.n_inliers = count;
        H.s12 = Stored(h.s);
        for (int i = 0; i < 9; i++) H.R12[i] = Stored(h.R[i]);
        for (int i = 0; i < 3; i++) H.t12[i] = Stored(h.t[i]);
        if (count >= best) { // the event rule: what iterate() returns on (:184-200)
            best = count;
            if (count > min_inliers) o.events[o.n_events++] = k;
        }
    }
    return o;
}

// ---------------------------------------------------------------------------------------------------------------- the reference's class
// The reference's interface on stored rows.  The rows -- of Sim3RansacHost or fetched from the device after
// orbfe_enqueue_sim3_ransac_batch -- hold every hypothesis the solver could ever compute, so iterate() only walks the events.
class Sim3Solver
{
public:
    // n1: keypoint slots of KF1 (vbInliers' size); the rows are referenced, not copied
    Sim3Solver(const Sim3Rows *rows, int n1, int minInliers = 20) : mRows(rows), mN1(n1) { SetRansacParameters(0.99, minInliers, rows->max_its); }

    // The iteration table that produced the rows was built from (probability, minInliers, maxIterations); this sets the same members
    // the reference's does.  mRansacMaxIts is the rows' n_its: the table's value for the N the filter found.
    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300)
    {
        mRansacProb = probability;
        mRansacMinInliers = minInliers;
        N = mRows->n_corr;
        mRansacMaxIts = std::max(1, std::min(mRows->n_its, maxIterations));
        mnIterations = 0;
        mNextEvent = 0;
        mBest = -1;
    }

    // returns the hypothesis the reference would return T12 of, or -1 (an empty cv::Mat)
    int iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers)
    {
        bNoMore = false;
        vbInliers = std::vector<bool>(mN1, false);
        nInliers = 0;
        if (N < mRansacMinInliers) {
            bNoMore = true;
            return -1;
        }
        const int end = std::min(mRansacMaxIts, mnIterations + std::max(nIterations, 0)); // the iterations this call may run
        while (mNextEvent < mRows->n_events && mRows->events[mNextEvent] < mnIterations) mNextEvent++;
        if (mNextEvent < mRows->n_events && mRows->events[mNextEvent] < end) {
            const int k = mRows->events[mNextEvent];
            mnIterations = k + 1;
            mBest = k;
            nInliers = mRows->hyp[k].n_inliers;
            const uint32_t *bits = &mRows->bits[(size_t)k * mRows->words];
            for (int i = 0; i < N; i++)
                if (bits[i >> 5] >> (i & 31) & 1u) vbInliers[mRows->corr[2 * (size_t)i]] = true;
            return k;
        }
        mnIterations = std::max(mnIterations, end);
        if (mnIterations >= mRansacMaxIts) bNoMore = true;
        return -1;
    }

    int find(std::vector<bool> &vbInliers12, int &nInliers)
    {
        bool bFlag;
        return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
    }

    // of the hypothesis iterate() returned last (the reference's mBest* after a return)
    const float *GetEstimatedRotation() const { return mRows->hyp[mBest].R12; }
    const float *GetEstimatedTranslation() const { return mRows->hyp[mBest].t12; }
    float GetEstimatedScale() const { return mRows->hyp[mBest].s12; }
    int Iterations() const { return mnIterations; }

private:
    const Sim3Rows *mRows;
    int mN1, N = 0, mRansacMinInliers = 0, mRansacMaxIts = 0, mnIterations = 0, mNextEvent = 0, mBest = -1;
    double mRansacProb = 0.99;
};

} // namespace ORB_SLAM2
