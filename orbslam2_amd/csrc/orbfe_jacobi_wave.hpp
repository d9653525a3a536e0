// orbfe_jacobi_wave.hpp -- cv::SVD::compute of an m x N float matrix (N <= 9 columns, m <= 16 rows) by one wave with At, Vt and W in LDS:
// the one-sided Jacobi of DESIGN.md section 4i2 (the per-lane 3 x 3 cv::Mat steps are in orbfe_cvmat.hpp).  Shared by
// orbfe_initializer_device.hip (the 8-point solutions and the rank-2 step) and orbfe_reconstruct_device.hip (DecomposeE and
// ReconstructH's decomposition): one definition, the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>

#define AT_STRIDE 16 // row stride of At
#define VT_STRIDE 9  // row stride of Vt

// ---------------------------------------------------------------------------------------------------------------- the Jacobi, in LDS
// one row of At (M floats, M a multiple of 4, 16-byte aligned) into registers: the address is wave-uniform, so the loads broadcast
template <int M> __device__ __forceinline__ void load_row(const float *row, float (&r)[M])
{
#pragma unroll
    for (int q = 0; q < M / 4; q++) {
        const float4 v = reinterpret_cast<const float4 *>(row)[q];
        r[4 * q] = v.x; r[4 * q + 1] = v.y; r[4 * q + 2] = v.z; r[4 * q + 3] = v.w;
    }
}

template <int M> __device__ __forceinline__ double square_sum(const float (&r)[M])
{
    double sd = 0;
#pragma unroll
    for (int k = 0; k < M; k++) sd += (double)r[k] * (double)r[k];
    return sd;
}

// cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) of an m x N float A (m <= M, rows m .. M - 1 of A ZERO: they change no bit) whose
// transpose is in At, by one wave.  On return W holds the singular values, descending, and the rows of At and Vt are carried by the
// selection sort.  Every lane reads both rows of a pair whole, evaluates p, the skip test, c, s, both rotated rows and their square sums
// in index order -- the same values in all lanes, so every branch is wave-uniform -- and writes back the one element it owns.
template <int N, int M> __device__ __forceinline__ void jacobi_wave(float *At, float *Vt, double *W, int lane)
{
    if (lane < N) {
        float r[M];
        load_row<M>(At + lane * AT_STRIDE, r);
        W[lane] = square_sum<M>(r);
        for (int k = 0; k < N; k++) Vt[lane * VT_STRIDE + k] = lane == k ? 1.f : 0.f;
    }
    __syncthreads();
    const double eps = (double)FLT_EPSILON * 2;
    const bool in_a = lane < M, in_v = lane >= 16 && lane < 16 + N;
    for (int iter = 0; iter < 30; iter++) {
        bool changed = false;
        for (int i = 0; i < N - 1; i++)
            for (int j = i + 1; j < N; j++) {
                float *Ai = At + i * AT_STRIDE, *Aj = At + j * AT_STRIDE;
                float *Xi = in_a ? Ai + lane : Vt + i * VT_STRIDE + (lane - 16), *Xj = in_a ? Aj + lane : Vt + j * VT_STRIDE + (lane - 16);
                float ai[M], aj[M], x = 0.f, y = 0.f;
                load_row<M>(Ai, ai);
                load_row<M>(Aj, aj);
                if (in_a || in_v) { x = *Xi; y = *Xj; }
                const double a = W[i], b = W[j];
                double p = 0;
#pragma unroll
                for (int k = 0; k < M; k++) p += (double)ai[k] * (double)aj[k];
                if (fabs(p) <= eps * sqrt(a * b)) continue;
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
                double na = 0, nb = 0;
#pragma unroll
                for (int k = 0; k < M; k++) {
                    const float t0 = __fadd_rn(__fmul_rn(c, ai[k]), __fmul_rn(s, aj[k]));
                    const float t1 = __fadd_rn(__fmul_rn(-s, ai[k]), __fmul_rn(c, aj[k]));
                    na += (double)t0 * (double)t0;
                    nb += (double)t1 * (double)t1;
                }
                const float o0 = __fadd_rn(__fmul_rn(c, x), __fmul_rn(s, y));
                const float o1 = __fadd_rn(__fmul_rn(-s, x), __fmul_rn(c, y));
                __syncthreads(); // every lane has read rows i and j
                if (in_a || in_v) { *Xi = o0; *Xj = o1; }
                if (lane == 0) { W[i] = na; W[j] = nb; }
                __syncthreads();
                changed = true;
            }
        if (!changed) break;
    }
    double w = 0;
    if (lane < N) {
        float r[M];
        load_row<M>(At + lane * AT_STRIDE, r);
        w = sqrt(square_sum<M>(r));
    }
    __syncthreads();
    if (lane < N) W[lane] = w;
    __syncthreads();
    for (int i = 0; i < N - 1; i++) {
        int j = i;
        for (int k = i + 1; k < N; k++)
            if (W[j] < W[k]) j = k;
        if (i != j) { // uniform
            const double wi = W[i], wj = W[j];
            float *Xi = in_a ? At + i * AT_STRIDE + lane : Vt + i * VT_STRIDE + (lane - 16), *Xj = in_a ? At + j * AT_STRIDE + lane : Vt + j * VT_STRIDE + (lane - 16);
            __syncthreads();
            if (in_a || in_v) { const float t = *Xi; *Xi = *Xj; *Xj = t; }
            if (lane == 0) { W[i] = wj; W[j] = wi; }
            __syncthreads();
        }
    }
}
