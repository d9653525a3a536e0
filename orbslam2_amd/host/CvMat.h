// CvMat.h -- the cv::Mat float rules that the host forms share, in plain C++: the one-sided Jacobi of
// cv::SVD::compute, the Mat product with its double sum and one rounding, Mat::inv / cv::determinant of a 3 x 3, cv::norm, the scale by
// (float)(1.0 / d) and the one stored NaN.  Header-only, no library, no OpenCV and no device needed.  Written literally, loops rolled:
// Initializer.h, Triangulate.h and MapPointUpdate.h are a second formulation next to the kernels' unrolled one, and these are their
// common steps (tests/cvmat_model.py is the model, tests/cvmat_mirror/mirror_main.cpp the driver that compares the two bit for bit).
// Compile with -ffp-contract=off: every float operation below is rounded once (contract Q4), as in the kernels.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <utility>

namespace ORB_SLAM2
{

enum { kCvMatAStride = 16, kCvMatVStride = 9 };

// The one-sided (Hestenes) Jacobi of cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) for an m x n float A, m >= n, held transposed:
// At[i * 16 + k] = A[k][i] (i < n <= 9, k < m <= 16), Vt[i * 9 + k].  On return W holds the singular values in descending order (strict
// selection sort) and the rows of At (the rotated columns, NOT normalised) and of Vt are carried with them.  Returns the number of
// sweeps that rotated.
inline int Jacobi(float *At, float *Vt, double *W, int n, int m)
{
    const int as = kCvMatAStride, vs = kCvMatVStride;
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) sd += (double)At[i * as + k] * At[i * as + k];
        W[i] = sd;
        for (int k = 0; k < n; k++) Vt[i * vs + k] = i == k ? 1.f : 0.f;
    }
    const double eps = (double)FLT_EPSILON * 2;
    int sweeps = 0;
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
        sweeps++;
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
    return sweeps;
}

// a cv::Mat product a[R][Kk] * b[Kk][C]: per element a double sum over k in index order, times *alpha when given (a MatExpr scale is
// the gemm's alpha), plus (double)plus[r][c] when given, rounded once
inline void MatMul(const float *a, const float *b, int R, int Kk, int C, float *out, const double *alpha = nullptr, const float *plus = nullptr)
{
    for (int r = 0; r < R; r++)
        for (int c = 0; c < C; c++) {
            double s = 0;
            for (int k = 0; k < Kk; k++) s += (double)a[Kk * r + k] * b[C * k + c];
            if (alpha) s = *alpha * s;
            if (plus) s += (double)plus[C * r + c];
            out[C * r + c] = (float)s;
        }
}

// cv::determinant of a 3x3 float matrix, in double
inline double Det3(const float m[9])
{
    const double m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5], m20 = m[6], m21 = m[7], m22 = m[8];
    return m00 * (m11 * m22 - m12 * m21) - m01 * (m10 * m22 - m12 * m20) + m02 * (m10 * m21 - m11 * m20);
}

// cv::Mat::inv() of a 3x3 float matrix (DECOMP_LU takes the closed form): determinant and cofactors in double, det == 0 gives zeros
inline void Inv3(const float m[9], float out[9])
{
    const double m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5], m20 = m[6], m21 = m[7], m22 = m[8];
    double d = Det3(m);
    if (d == 0) {
        for (int k = 0; k < 9; k++) out[k] = 0.f;
        return;
    }
    d = 1. / d;
    out[0] = (float)((m11 * m22 - m12 * m21) * d); out[1] = (float)((m02 * m21 - m01 * m22) * d); out[2] = (float)((m01 * m12 - m02 * m11) * d);
    out[3] = (float)((m12 * m20 - m10 * m22) * d); out[4] = (float)((m00 * m22 - m02 * m20) * d); out[5] = (float)((m02 * m10 - m00 * m12) * d);
    out[6] = (float)((m10 * m21 - m11 * m20) * d); out[7] = (float)((m01 * m20 - m00 * m21) * d); out[8] = (float)((m00 * m11 - m01 * m10) * d);
}

// cv::SVD::compute of a 3x3 float matrix: the Jacobi on its columns; w[i] = (float)W[i], u[k][i] = At[i][k] * (float)(1 / W[i]), 0 when
// W[i] <= FLT_MIN (the basis completion of a zero singular value is not restated)
inline void Svd3(const float A[9], float u[9], float w[3], float vt[9])
{
    float At[3 * kCvMatAStride], Vt[3 * kCvMatVStride];
    double W[3];
    for (int i = 0; i < 3; i++)
        for (int k = 0; k < 3; k++) At[i * kCvMatAStride + k] = A[3 * k + i];
    Jacobi(At, Vt, W, 3, 3);
    for (int i = 0; i < 3; i++) {
        const float s = W[i] > (double)FLT_MIN ? (float)(1 / W[i]) : 0.f;
        w[i] = (float)W[i];
        for (int k = 0; k < 3; k++) { u[3 * k + i] = At[i * kCvMatAStride + k] * s; vt[3 * i + k] = Vt[i * kCvMatVStride + k]; }
    }
}

// cv::norm of a 3-vector of floats: a double sum of double squares in index order, one sqrt
inline double Norm3(const float v[3])
{
    double s = 0;
    for (int k = 0; k < 3; k++) s += (double)v[k] * v[k];
    return std::sqrt(s);
}

// t / cv::norm(t): a scale by (float)(1.0 / norm); no zero test
inline void Unit(float t[3])
{
    const float a = (float)(1.0 / Norm3(t));
    for (int k = 0; k < 3; k++) t[k] = t[k] * a;
}

// cv::reduce(., CV_REDUCE_SUM) of n floats: a float sum in index order
inline float ReduceSum(const float *v, int n)
{
    float s = v[0];
    for (int k = 1; k < n; k++) s = s + v[k];
    return s;
}

// Mat::dot of two float matrices of n elements: a double sum of double products in index order
inline double Dot(const float *a, const float *b, int n)
{
    double s = 0;
    for (int k = 0; k < n; k++) s += (double)a[k] * b[k];
    return s;
}

// cv::pow(., 2) on floats is a float product; the element-wise `den += aux.at<float>(i, j)` over it a double sum of those float squares
inline double SumOfSquaredFloats(const float *v, int n)
{
    double s = 0;
    for (int k = 0; k < n; k++) {
        const float sq = v[k] * v[k];
        s += sq;
    }
    return s;
}

// float = double / double (ms12i = nom / den): the double quotient rounded once; den == 0 is IEEE
inline float Ratio(double nom, double den) { return (float)(nom / den); }

// a NaN is stored with one bit pattern everywhere
inline float Stored(float s)
{
    if (s != s) { const uint32_t q = 0x7fc00000u; std::memcpy(&s, &q, 4); }
    return s;
}

// ---------------------------------------------------------------------------------------------------------------- the double rules
// The CV_64F steps of the C interface that EPnP (host/PnPsolver.h) calls: cvMulTransposed, cvSVD, cvSolve and cvInvert with CV_SVD.
// DESIGN.md sections 4i2 and 4p state them.  These functions carry ORBFE_CV_HD: orbfe_pnp_ransac.hip compiles this one definition for the
// device as well, so the kernels and the host form cannot differ in an operation or its order.
#ifndef ORBFE_CV_HD
#ifdef __HIPCC__
#define ORBFE_CV_HD __host__ __device__
#else
#define ORBFE_CV_HD
#endif
#endif

// cvMulTransposed(M, MtM, 1) one row of M at a time: acc (n x n, row-major, zero before the first row) gains row^T row in its upper
// triangle, so every element is a double sum over the rows in index order; MulTransposedMirror then copies the upper triangle down
ORBFE_CV_HD inline void MulTransposedAdd(double *acc, const double *row, int n)
{
    for (int a = 0; a < n; a++)
        for (int b = a; b < n; b++) acc[a * n + b] += row[a] * row[b];
}

ORBFE_CV_HD inline void MulTransposedMirror(double *acc, int n)
{
    for (int a = 1; a < n; a++)
        for (int b = 0; b < a; b++) acc[a * n + b] = acc[b * n + a];
}

// Jacobi above instantiated in double (cv::SVD of a CV_64F matrix): At[i * as + k] = A[k][i] (i < n, k < m), Vt[i * vs + k] or NULL where
// the caller reads no V.  eps = DBL_EPSILON * 10, at most 30 sweeps, the strict selection sort.  The rows of At are NOT normalised.
ORBFE_CV_HD inline int JacobiD(double *At, int as, double *Vt, int vs, double *W, int n, int m)
{
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) sd += At[i * as + k] * At[i * as + k];
        W[i] = sd;
        if (Vt)
            for (int k = 0; k < n; k++) Vt[i * vs + k] = i == k ? 1.0 : 0.0;
    }
    const double eps = DBL_EPSILON * 10;
    int sweeps = 0;
    for (int iter = 0; iter < 30; iter++) {
        bool changed = false;
        for (int i = 0; i < n - 1; i++)
            for (int j = i + 1; j < n; j++) {
                double *Ai = At + i * as, *Aj = At + j * as;
                double a = W[i], b = W[j], p = 0;
                for (int k = 0; k < m; k++) p += Ai[k] * Aj[k];
                if (std::fabs(p) <= eps * std::sqrt(a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = std::sqrt(p * p + beta * beta); // not hypot
                double c, s;
                if (beta < 0) {
                    s = std::sqrt(((gamma - beta) * 0.5) / gamma);
                    c = p / (gamma * s * 2);
                } else {
                    c = std::sqrt((gamma + beta) / (gamma * 2));
                    s = p / (gamma * c * 2);
                }
                a = b = 0;
                for (int k = 0; k < m; k++) {
                    const double t0 = c * Ai[k] + s * Aj[k];
                    const double t1 = -s * Ai[k] + c * Aj[k];
                    Ai[k] = t0; Aj[k] = t1;
                    a += t0 * t0; b += t1 * t1;
                }
                W[i] = a; W[j] = b;
                changed = true;
                if (Vt) {
                    double *Vi = Vt + i * vs, *Vj = Vt + j * vs;
                    for (int k = 0; k < n; k++) {
                        const double t0 = c * Vi[k] + s * Vj[k];
                        const double t1 = -s * Vi[k] + c * Vj[k];
                        Vi[k] = t0; Vj[k] = t1;
                    }
                }
            }
        if (!changed) break;
        sweeps++;
    }
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) sd += At[i * as + k] * At[i * as + k];
        W[i] = std::sqrt(sd);
    }
    for (int i = 0; i < n - 1; i++) {
        int j = i;
        for (int k = i + 1; k < n; k++)
            if (W[j] < W[k]) j = k;
        if (i != j) {
            double t = W[i]; W[i] = W[j]; W[j] = t;
            for (int k = 0; k < m; k++) { t = At[i * as + k]; At[i * as + k] = At[j * as + k]; At[j * as + k] = t; }
            if (Vt)
                for (int k = 0; k < n; k++) { t = Vt[i * vs + k]; Vt[i * vs + k] = Vt[j * vs + k]; Vt[j * vs + k] = t; }
        }
    }
    return sweeps;
}

// the left singular vectors: u_i = At_i * (1 / W_i), the zero row where W_i <= DBL_MIN (OpenCV completes such a row with random
// vectors; that is not restated)
ORBFE_CV_HD inline void JacobiUnitRowsD(double *At, int as, const double *W, int n, int m)
{
    for (int i = 0; i < n; i++) {
        const double s = W[i] > DBL_MIN ? 1 / W[i] : 0.0;
        for (int k = 0; k < m; k++) At[i * as + k] = At[i * as + k] * s;
    }
}

// cvSVD(A, W, Ut, Vt', MODIFY_A | U_T) of a square n x n double matrix A (row-major, n <= 12): w descending, the rows of Ut the left
// singular vectors, the rows of Vt (or NULL) the right ones
ORBFE_CV_HD inline int SvdSquareD(const double *A, int n, double *w, double *Ut, double *Vt)
{
    for (int i = 0; i < n; i++)
        for (int k = 0; k < n; k++) Ut[i * n + k] = A[k * n + i];
    const int sweeps = JacobiD(Ut, n, Vt, n, w, n, n);
    JacobiUnitRowsD(Ut, n, w, n, n);
    return sweeps;
}

// SVBkSb: x (n) = sum over i of ((u_i . b) / w_i) v_i in index order, the terms with w_i <= 2 * DBL_EPSILON * sum(w) left out.
// Ut: n unit rows of m, Vt: n rows of n.  b == NULL stands for column `unit` of the identity (cvInvert): u_i . b is then Ut[i][unit].
ORBFE_CV_HD inline void SvBkSbD(const double *Ut, int us, const double *Vt, int vs, const double *w, int n, int m, const double *b, int unit, double *x)
{
    double sum = 0;
    for (int i = 0; i < n; i++) sum += w[i];
    const double threshold = 2 * DBL_EPSILON * sum;
    for (int j = 0; j < n; j++) x[j] = 0;
    for (int i = 0; i < n; i++) {
        if (w[i] <= threshold) continue;
        double s = 0;
        if (b)
            for (int k = 0; k < m; k++) s += Ut[i * us + k] * b[k];
        else
            s = Ut[i * us + unit];
        s = s / w[i];
        for (int j = 0; j < n; j++) x[j] += s * Vt[i * vs + j];
    }
}

// cvSolve(A, b, x, CV_SVD) of an m x n double A (row-major, m = 6, n <= 5): the Jacobi on A's columns, then the back-substitution
ORBFE_CV_HD inline void SolveSvdD(const double *A, int m, int n, const double *b, double *x, double *w)
{
    double At[5 * 6], Vt[5 * 5];
    for (int i = 0; i < n; i++)
        for (int k = 0; k < m; k++) At[i * 6 + k] = A[k * n + i];
    JacobiD(At, 6, Vt, 5, w, n, m);
    JacobiUnitRowsD(At, 6, w, n, m);
    SvBkSbD(At, 6, Vt, 5, w, n, m, b, 0, x);
}

// cvInvert(A, inv, CV_SVD) of a 3 x 3 double A: the pseudo-inverse by the same two steps, column by column
ORBFE_CV_HD inline void InvertSvd3D(const double A[9], double inv[9], double w[3])
{
    double Ut[9], Vt[9], x[3];
    SvdSquareD(A, 3, w, Ut, Vt);
    for (int k = 0; k < 3; k++) {
        SvBkSbD(Ut, 3, Vt, 3, w, 3, 3, nullptr, k, x);
        for (int j = 0; j < 3; j++) inv[3 * j + k] = x[j];
    }
}

} // namespace ORB_SLAM2
