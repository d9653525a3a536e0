// orbfe_cvmat.hpp -- the per-lane cv::Mat float steps of DESIGN.md section 4i2 on 3 x 3 matrices and 3-vectors in registers: the product
// (a double sum over k in index order, one rounding) with its alpha and `+ C` forms, Mat::inv / cv::determinant, cv::norm, the scale by
// (float)(1.0 / d), cv::reduce / Mat::dot / the sum of cv::pow(., 2) on a 3 x 3, and the one stored NaN.  Shared by
// orbfe_initializer_device.hip, orbfe_reconstruct_device.hip, orbfe_triangulate_device.hip and orbfe_sim3_ransac.hip: one definition, the same bits.  The Jacobis are in orbfe_jacobi4.hpp and orbfe_jacobi_wave.hpp.
#pragma once
#include <hip/hip_runtime.h>

// ---------------------------------------------------------------------------------------------------------------- 3 x 3 products
// a cv::Mat product: per element a double sum over k in index order, rounded once
__device__ __forceinline__ void mul3(const float (&a)[9], const float (&b)[9], float (&out)[9])
{
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            double s = 0;
#pragma unroll
            for (int k = 0; k < 3; k++) s += (double)a[3 * r + k] * (double)b[3 * k + c];
            out[3 * r + c] = (float)s;
        }
}

// cv::Mat::inv() of a 3 x 3 float matrix: determinant and cofactors in double; det == 0 gives the zero matrix
__device__ __forceinline__ void inv3(const float (&m)[9], float (&out)[9])
{
    const double m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5], m20 = m[6], m21 = m[7], m22 = m[8];
    double d = m00 * (m11 * m22 - m12 * m21) - m01 * (m10 * m22 - m12 * m20) + m02 * (m10 * m21 - m11 * m20);
    if (d == 0) {
#pragma unroll
        for (int k = 0; k < 9; k++) out[k] = 0.f;
        return;
    }
    d = 1. / d;
    out[0] = (float)((m11 * m22 - m12 * m21) * d); out[1] = (float)((m02 * m21 - m01 * m22) * d); out[2] = (float)((m01 * m12 - m02 * m11) * d);
    out[3] = (float)((m12 * m20 - m10 * m22) * d); out[4] = (float)((m00 * m22 - m02 * m20) * d); out[5] = (float)((m02 * m10 - m00 * m12) * d);
    out[6] = (float)((m10 * m21 - m11 * m20) * d); out[7] = (float)((m01 * m20 - m00 * m21) * d); out[8] = (float)((m00 * m11 - m01 * m10) * d);
}

// cv::determinant of a 3 x 3 float matrix: the double expression d of inv3
__device__ __forceinline__ double det3(const float (&m)[9])
{
    const double m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5], m20 = m[6], m21 = m[7], m22 = m[8];
    return m00 * (m11 * m22 - m12 * m21) - m01 * (m10 * m22 - m12 * m20) + m02 * (m10 * m21 - m11 * m20);
}

// (alpha * a) * b as one gemm: the double sum times alpha, rounded once
__device__ __forceinline__ void mul3_alpha(double alpha, const float (&a)[9], const float (&b)[9], float (&out)[9])
{
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            double s = 0;
#pragma unroll
            for (int k = 0; k < 3; k++) s += (double)a[3 * r + k] * (double)b[3 * k + c];
            out[3 * r + c] = (float)(alpha * s);
        }
}

// a (3 x 3) * v (3 x 1)
__device__ __forceinline__ void mul3_vec(const float (&a)[9], const float (&v)[3], float (&out)[3])
{
#pragma unroll
    for (int r = 0; r < 3; r++) {
        double s = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) s += (double)a[3 * r + k] * (double)v[k];
        out[r] = (float)s;
    }
}

// the float sqrt of :607-650, correctly rounded: the double sqrt is IEEE and rounding it once more changes nothing for a float argument
// (the __fsqrt_rn intrinsic is the hardware's approximation)
__device__ __forceinline__ float sqrt_rn(float x) { return (float)sqrt((double)x); }

// t / cv::norm(t): a scale by (float)(1.0 / norm); no zero test
__device__ __forceinline__ void unit3(float (&t)[3])
{
    const double d = sqrt((double)t[0] * (double)t[0] + (double)t[1] * (double)t[1] + (double)t[2] * (double)t[2]);
    const float a = (float)(1.0 / d);
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = __fmul_rn(t[k], a);
}

// ---------------------------------------------------------------------------------------------------------------- products on a Tcw of 12 floats
// Rwc * x (+ Ow): Rwc[i][k] = Tcw[k][i]; a double sum over k, one rounding
__device__ __forceinline__ void rwc_times(const float (&Tcw)[12], const float (&x)[3], const float *plus, float (&out)[3])
{
#pragma unroll
    for (int i = 0; i < 3; i++) {
        double s = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) s += (double)Tcw[4 * k + i] * (double)x[k];
        if (plus) s += (double)plus[i];
        out[i] = (float)s;
    }
}

// Rcw.row(R).dot(x3Dt) + tcw(R)
template <int R> __device__ __forceinline__ float row_dot_plus(const float (&Tcw)[12], const float (&X)[3])
{
    double s = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) s += (double)Tcw[4 * R + k] * (double)X[k];
    return (float)(s + (double)Tcw[4 * R + 3]);
}

__device__ __forceinline__ double norm3(const float (&v)[3])
{
    return sqrt((double)v[0] * (double)v[0] + (double)v[1] * (double)v[1] + (double)v[2] * (double)v[2]);
}

// ---------------------------------------------------------------------------------------------------------------- reductions of a 3 x 3
// cv::reduce(., CV_REDUCE_SUM) along a row of three floats: a float sum in index order
__device__ __forceinline__ float reduce_sum3(float a, float b, float c) { return (a + b) + c; }

// Mat::dot of two 3 x 3 float matrices: a double sum of double products in index order
__device__ __forceinline__ double dot9(const float (&a)[9], const float (&b)[9])
{
    double s = 0;
#pragma unroll
    for (int k = 0; k < 9; k++) s += (double)a[k] * (double)b[k];
    return s;
}

// cv::pow(., 2) on floats is a float product; summing its elements into a double is a double sum of those float squares
__device__ __forceinline__ double sum_of_squared_floats9(const float (&v)[9])
{
    double s = 0;
#pragma unroll
    for (int k = 0; k < 9; k++) s += (double)__fmul_rn(v[k], v[k]);
    return s;
}

// float = double / double: the double quotient rounded once; den == 0 is IEEE
__device__ __forceinline__ float ratio(double nom, double den) { return (float)(nom / den); }

// ---------------------------------------------------------------------------------------------------------------- stored floats
__device__ __forceinline__ float one_nan(float v) { return v != v ? __int_as_float(0x7fc00000) : v; } // a NaN is stored with one bit pattern

__device__ __forceinline__ bool finite(float v) { return fabsf(v) < __int_as_float(0x7f800000); }
