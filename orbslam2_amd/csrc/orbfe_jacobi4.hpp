// orbfe_jacobi4.hpp -- vt.row(3) of cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) for a 4 x 4 float A, per lane in registers: the
// one-sided Jacobi of DESIGN.md section 4k.  The six (i, j) rotations are instantiated with static indices and the selection sort
// carries values, not indices, so At, Vt and W never leave the registers.  Shared by orbfe_triangulate_device.hip (CreateNewMapPoints)
// and orbfe_reconstruct_device.hip (Initializer::Triangulate inside CheckRT): one definition, the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>

// ---------------------------------------------------------------------------------------------------------------- the null vector
struct Jacobi {
    float At[4][4], Vt[4][4];
    double W[4];
};

// rows I and J of X rotated in float: t0 = c * a + s * b, t1 = -s * a + c * b, each product rounded, then the sum
template <int I, int J> __device__ __forceinline__ void rotate_rows(float (&X)[4][4], float c, float s)
{
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float t0 = __fadd_rn(__fmul_rn(c, X[I][k]), __fmul_rn(s, X[J][k]));
        const float t1 = __fadd_rn(__fmul_rn(-s, X[I][k]), __fmul_rn(c, X[J][k]));
        X[I][k] = t0; X[J][k] = t1;
    }
}

template <int I> __device__ __forceinline__ double square_sum(const float (&X)[4][4])
{
    double sd = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) sd += (double)X[I][k] * (double)X[I][k];
    return sd;
}

template <int I, int J> __device__ __forceinline__ bool jacobi_pair(Jacobi &m)
{
    const double a = m.W[I], b = m.W[J];
    double p = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) p += (double)m.At[I][k] * (double)m.At[J][k];
    const double eps = (double)FLT_EPSILON * 2;
    if (fabs(p) <= eps * sqrt(a * b)) return false;
    p *= 2;
    const double beta = a - b, gamma = sqrt(p * p + beta * beta); // a plain double sqrt, not hypot
    float c, s;
    if (beta < 0) {
        s = (float)sqrt(((gamma - beta) * 0.5) / gamma);
        c = (float)(p / (gamma * (double)s * 2));
    } else {
        c = (float)sqrt((gamma + beta) / (gamma * 2));
        s = (float)(p / (gamma * (double)c * 2));
    }
    rotate_rows<I, J>(m.At, c, s);
    m.W[I] = square_sum<I>(m.At);
    m.W[J] = square_sum<J>(m.At);
    rotate_rows<I, J>(m.Vt, c, s);
    return true;
}

// position I of the selection sort (descending, strict <): the largest of W[I..3] comes to I and carries its row of Vt
template <int I> __device__ __forceinline__ void select_largest(Jacobi &m)
{
    int j = I;
    double wj = m.W[I];
#pragma unroll
    for (int k = I + 1; k < 4; k++)
        if (wj < m.W[k]) { j = k; wj = m.W[k]; }
#pragma unroll
    for (int k = I + 1; k < 4; k++)
        if (j == k) {
            const double t = m.W[I]; m.W[I] = m.W[k]; m.W[k] = t;
#pragma unroll
            for (int e = 0; e < 4; e++) { const float u = m.Vt[I][e]; m.Vt[I][e] = m.Vt[k][e]; m.Vt[k][e] = u; }
        }
}

// vt.row(3) of cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV): m.At holds A transposed on entry
__device__ __forceinline__ void null_vector(Jacobi &m, float (&v)[4])
{
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int k = 0; k < 4; k++) m.Vt[i][k] = i == k ? 1.f : 0.f;
    m.W[0] = square_sum<0>(m.At); m.W[1] = square_sum<1>(m.At); m.W[2] = square_sum<2>(m.At); m.W[3] = square_sum<3>(m.At);
    for (int iter = 0; iter < 30; iter++) {
        bool changed = jacobi_pair<0, 1>(m);
        changed |= jacobi_pair<0, 2>(m);
        changed |= jacobi_pair<0, 3>(m);
        changed |= jacobi_pair<1, 2>(m);
        changed |= jacobi_pair<1, 3>(m);
        changed |= jacobi_pair<2, 3>(m);
        if (!changed) break;
    }
    m.W[0] = sqrt(square_sum<0>(m.At)); m.W[1] = sqrt(square_sum<1>(m.At)); m.W[2] = sqrt(square_sum<2>(m.At)); m.W[3] = sqrt(square_sum<3>(m.At));
    select_largest<0>(m);
    select_largest<1>(m);
    select_largest<2>(m);
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = m.Vt[3][k];
}
