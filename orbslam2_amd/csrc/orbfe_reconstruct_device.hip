// orbfe_reconstruct_device.hip -- Initializer::ReconstructF / ReconstructH with DecomposeE, CheckRT and Triangulate
// (src/Initializer.cc:469-746, :797-928) and the RH test of Initialize (:111-117) on what orbfe_enqueue_find_homography_fundamental left
// in HBM, asynchronous on the caller's stream.  The entry points and their checks are at the end of this file; the arithmetic contract is
// stated in include/orbfe.h and DESIGN.md section 4m, and this file, orbslam2_amd/host/Initializer.h and tests/reconstruct_model.py follow
// it operation by operation.
//
//   reconstruct_hypotheses_kernel   one wave.  Takes the RH decision, computes E21 = K.t() F21 K or A = K.inv() H21 K and its 3 x 3 Jacobi
//                                   in LDS (the wave-wide routine of the RANSAC), then lane h < 8 builds motion hypothesis h with selects in
//                                   place of the reference's tables, writes (R, t) out and (R, t, P2 = K [R|t], O2 = -R.t() t) to the context's
//                                   scratch.  The early results 1 (no RANSAC winner) and 2 (the test of :596) are taken here.
//   reconstruct_check_kernel        one lane per (match, hypothesis); the hypothesis is the grid's second dimension, so a wave never mixes
//                                   hypotheses and the record of its hypothesis is loaded through wave-uniform addresses.  The 4 x 4 Jacobi
//                                   runs in registers (orbfe_jacobi4.hpp).  Writes a code and a cosine per entry.
//   reconstruct_select_kernel       one workgroup: counts per hypothesis, the k-th smallest cosine by a 4 x 8-bit radix select on
//                                   order-preserving keys (as stereo_median_kernel), the count rules, the clearing of d_p3d / d_triangulated
//                                   and the chosen hypothesis's points, evaluated a second time with the same operations.
// All stores are plain vector stores.
#include "../../include/orbfe.h"
#include "orbfe_config.h"
#include "orbfe_host.h"
#include "../host/Initializer.h"
#include "orbfe_cvmat.hpp"
#include "orbfe_jacobi4.hpp"
#include "orbfe_jacobi_wave.hpp"

#include <cfloat>

#define HYP_FLOATS 27 // R[9], t[3], P2[12], O2[3]

// what every kernel of this file takes.  head, hyp, cos and (without d_codes) codes are the context's scratch.
struct orbfe_reconstruct_args {
    const orbfe_keypoint *keys1, *keys2;
    const int32_t *pairs;
    const float *H21, *F21, *score;
    const int32_t *best;
    const uint8_t *inl_h, *inl_f;
    int n1, n2, N, min_triangulated, model;
    float K4[4], th2;
    int32_t *out_model;
    float *hyp_R, *hyp_t;
    int32_t *ngood;
    float *cos_parallax;
    int32_t *result, *choice;
    float *R21, *t21, *p3d;
    uint8_t *triangulated, *codes;
    int32_t *status;
    int32_t *head; // nhyp, model, early result
    float *hyp;    // [8][HYP_FLOATS]
    float *cos;    // [8][N]
};
typedef orbfe_reconstruct_args Args;

static_assert(sizeof(orbfe_keypoint) == 28, "orbfe_keypoint");

// ---------------------------------------------------------------------------------------------------------------- the hypotheses
// cv::SVD::compute of the 3 x 3 A that every lane holds: u, w, vt in every lane
__device__ __forceinline__ void svd3_wave(const float (&A)[9], float *At, float *Vt, double *W, int lane, float (&u)[9], float (&w)[3], float (&vt)[9])
{
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int k = 0; k < 3; k++) At[i * AT_STRIDE + k] = A[3 * k + i];
            At[i * AT_STRIDE + 3] = 0.f; // the fourth, zero row of the 3 x 3 problem
        }
    }
    __syncthreads();
    jacobi_wave<3, 4>(At, Vt, W, lane);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double wi = W[i];
        const float s = wi > (double)FLT_MIN ? (float)(1 / wi) : 0.f;
        w[i] = (float)wi;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            u[3 * k + i] = __fmul_rn(At[i * AT_STRIDE + k], s);
            vt[3 * i + k] = Vt[i * VT_STRIDE + k];
        }
    }
}

__global__ __launch_bounds__(64) void reconstruct_hypotheses_kernel(Args a)
{
    __shared__ __attribute__((aligned(16))) float At[3 * AT_STRIDE];
    __shared__ float Vt[3 * VT_STRIDE];
    __shared__ double W[3];
    const int lane = threadIdx.x;
    int model = a.model;
    if (model < 0) { // :111-117
        const float SH = a.score[0], SF = a.score[1];
        const float RH = __fdiv_rn(SH, __fadd_rn(SH, SF));
        model = (double)RH > 0.40 ? 0 : 1;
    }
    const bool winner = a.best[model] >= 0;
    if (lane == 0) {
        *a.out_model = model;
        a.head[1] = model;
    }
    if (!winner) {
        if (lane == 0) { a.head[0] = 0; a.head[2] = 1; }
        return;
    }
    const float fx = a.K4[0], fy = a.K4[1], cx = a.K4[2], cy = a.K4[3];
    const float K[9] = {fx, 0.f, cx, 0.f, fy, cy, 0.f, 0.f, 1.f};
    float M[9], T[9], A[9], u[9], w[3], vt[9];
    const float *src = model == 0 ? a.H21 : a.F21;
#pragma unroll
    for (int k = 0; k < 9; k++) M[k] = src[k];
    float R[9], t[3];
    int nhyp;
    const int h = lane & 7, i = h & 3;
    if (model == 1) { // ReconstructF (:478-496) with DecomposeE (:908-928)
        const float Kt[9] = {fx, 0.f, 0.f, 0.f, fy, 0.f, cx, cy, 1.f};
        mul3(Kt, M, T);
        mul3(T, K, A); // E21 = K.t() * F21 * K
        svd3_wave(A, At, Vt, W, lane, u, w, vt);
        t[0] = u[2]; t[1] = u[5]; t[2] = u[8];
        unit3(t);
        const float Wm[9] = {0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f}, Wt[9] = {0.f, 1.f, 0.f, -1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
        float R1[9], R2[9];
        mul3(u, Wm, T);
        mul3(T, vt, R1);
        const bool neg1 = det3(R1) < 0;
        mul3(u, Wt, T);
        mul3(T, vt, R2);
        const bool neg2 = det3(R2) < 0;
#pragma unroll
        for (int k = 0; k < 9; k++) {
            const float r1 = neg1 ? -R1[k] : R1[k], r2 = neg2 ? -R2[k] : R2[k];
            R[k] = (h & 1) ? r2 : r1;
        }
        if (h & 2) { t[0] = -t[0]; t[1] = -t[1]; t[2] = -t[2]; }
        nhyp = 4;
    } else {          // ReconstructH (:583-685)
        float Ki[9];
        inv3(K, Ki);
        mul3(Ki, M, T);
        mul3(T, K, A); // A = invK * H21 * K
        svd3_wave(A, At, Vt, W, lane, u, w, vt);
        const float s = (float)(det3(u) * det3(vt));
        const float d1 = w[0], d2 = w[1], d3 = w[2];
        if ((double)__fdiv_rn(d1, d2) < 1.00001 || (double)__fdiv_rn(d2, d3) < 1.00001) {
            if (lane == 0) { a.head[0] = 0; a.head[2] = 2; }
            return;
        }
        const float q1 = __fmul_rn(d1, d1), q2 = __fmul_rn(d2, d2), q3 = __fmul_rn(d3, d3);
        const float aux1 = sqrt_rn(__fdiv_rn(__fsub_rn(q1, q2), __fsub_rn(q1, q3)));
        const float aux3 = sqrt_rn(__fdiv_rn(__fsub_rn(q2, q3), __fsub_rn(q1, q3)));
        const float x1 = i < 2 ? aux1 : -aux1, x3 = (i & 1) ? -aux3 : aux3;
        const float root = sqrt_rn(__fmul_rn(__fsub_rn(q1, q2), __fsub_rn(q2, q3)));
        const bool plus = i == 0 || i == 3;
        float Rp[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, tp[3];
        if (h < 4) { // case d' = d2
            const float den = __fmul_rn(__fadd_rn(d1, d3), d2);
            const float aux_stheta = __fdiv_rn(root, den), ctheta = __fdiv_rn(__fadd_rn(q2, __fmul_rn(d1, d3)), den);
            const float st = plus ? aux_stheta : -aux_stheta;
            Rp[0] = ctheta; Rp[2] = -st; Rp[6] = st; Rp[8] = ctheta;
            const float f = __fsub_rn(d1, d3);
            tp[0] = __fmul_rn(x1, f); tp[1] = __fmul_rn(0.f, f); tp[2] = __fmul_rn(-x3, f);
        } else {     // case d' = -d2
            const float den = __fmul_rn(__fsub_rn(d1, d3), d2);
            const float aux_sphi = __fdiv_rn(root, den), cphi = __fdiv_rn(__fsub_rn(__fmul_rn(d1, d3), q2), den);
            const float sp = plus ? aux_sphi : -aux_sphi;
            Rp[0] = cphi; Rp[2] = sp; Rp[4] = -1.f; Rp[6] = sp; Rp[8] = -cphi;
            const float f = __fadd_rn(d1, d3);
            tp[0] = __fmul_rn(x1, f); tp[1] = __fmul_rn(0.f, f); tp[2] = __fmul_rn(x3, f);
        }
        mul3_alpha((double)s, u, Rp, T); // s * U * Rp: the scale is the gemm's alpha (OPENCV-4.5.5-SEMANTICS)
        mul3(T, vt, R);
        mul3_vec(u, tp, t);
        unit3(t);
        nhyp = 8;
    }
    if (lane == 0) { a.head[0] = nhyp; a.head[2] = 0; }
    if (lane >= nhyp) return;
    // CheckRT's camera 2 (:819-825): P2 = K * [R|t], O2 = -R.t() * t
    float *rec = a.hyp + h * HYP_FLOATS;
#pragma unroll
    for (int k = 0; k < 9; k++) { rec[k] = R[k]; a.hyp_R[9 * h + k] = one_nan(R[k]); }
#pragma unroll
    for (int k = 0; k < 3; k++) { rec[9 + k] = t[k]; a.hyp_t[3 * h + k] = one_nan(t[k]); }
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            double s = 0;
#pragma unroll
            for (int k = 0; k < 3; k++) s += (double)K[3 * r + k] * (double)(c < 3 ? R[3 * k + c] : t[k]);
            rec[12 + 4 * r + c] = (float)s;
        }
#pragma unroll
    for (int r = 0; r < 3; r++) {
        double s = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) s += (double)R[3 * k + r] * (double)t[k];
        rec[24 + r] = (float)(-1.0 * s);
    }
}

// ---------------------------------------------------------------------------------------------------------------- CheckRT
__device__ __forceinline__ bool pair_ok(const Args &a, int i1, int i2) { return i1 >= 0 && i1 < a.n1 && i2 >= 0 && i2 < a.n2; }

// one iteration of CheckRT's loop (:829-893) for an inlier match under the hypothesis record `rec`: the code (1 .. 7), the cosine, the point
__device__ __forceinline__ int check_match(const float *rec, const float (&K4)[4], float x1, float y1, float x2, float y2, float th2, float &cosp, float (&p)[3])
{
    const float fx = K4[0], fy = K4[1], cx = K4[2], cy = K4[3];
    float R[9], t[3], P2[12], O2[3];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = rec[k];
#pragma unroll
    for (int k = 0; k < 3; k++) { t[k] = rec[9 + k]; O2[k] = rec[24 + k]; }
#pragma unroll
    for (int k = 0; k < 12; k++) P2[k] = rec[12 + k];
    const float P1[12] = {fx, 0.f, cx, 0.f, 0.f, fy, cy, 0.f, 0.f, 0.f, 1.f, 0.f};
    // Triangulate (:733-746): A.row(r) = x * P.row(2) - P.row(r'), held transposed
    Jacobi m;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        m.At[c][0] = __fsub_rn(__fmul_rn(x1, P1[8 + c]), P1[c]);
        m.At[c][1] = __fsub_rn(__fmul_rn(y1, P1[8 + c]), P1[4 + c]);
        m.At[c][2] = __fsub_rn(__fmul_rn(x2, P2[8 + c]), P2[c]);
        m.At[c][3] = __fsub_rn(__fmul_rn(y2, P2[8 + c]), P2[4 + c]);
    }
    float v[4];
    null_vector(m, v);
    const float alpha = (float)(1.0 / (double)v[3]); // no zero test: the reference has none
    p[0] = __fmul_rn(v[0], alpha); p[1] = __fmul_rn(v[1], alpha); p[2] = __fmul_rn(v[2], alpha);
    cosp = 0.f;
    if (!finite(p[0]) || !finite(p[1]) || !finite(p[2])) return 1;
    // Check parallax
    float n2[3];
    double s1 = 0, s2 = 0, dot = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        n2[k] = __fsub_rn(p[k], O2[k]);
        s1 += (double)p[k] * (double)p[k]; s2 += (double)n2[k] * (double)n2[k]; dot += (double)p[k] * (double)n2[k];
    }
    const float dist1 = (float)sqrt(s1), dist2 = (float)sqrt(s2);
    cosp = (float)(dot / (double)__fmul_rn(dist1, dist2));
    const bool low = (double)cosp < 0.99998;
    if (p[2] <= 0 && low) return 2;
    float p2[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        double s = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) s += (double)R[3 * r + k] * (double)p[k];
        p2[r] = (float)(s + (double)t[r]);
    }
    if (p2[2] <= 0 && low) return 3;
    const float invz1 = (float)(1.0 / (double)p[2]);
    const float ex1 = __fsub_rn(__fadd_rn(__fmul_rn(__fmul_rn(fx, p[0]), invz1), cx), x1), ey1 = __fsub_rn(__fadd_rn(__fmul_rn(__fmul_rn(fy, p[1]), invz1), cy), y1);
    if (__fadd_rn(__fmul_rn(ex1, ex1), __fmul_rn(ey1, ey1)) > th2) return 4;
    const float invz2 = (float)(1.0 / (double)p2[2]);
    const float ex2 = __fsub_rn(__fadd_rn(__fmul_rn(__fmul_rn(fx, p2[0]), invz2), cx), x2), ey2 = __fsub_rn(__fadd_rn(__fmul_rn(__fmul_rn(fy, p2[1]), invz2), cy), y2);
    if (__fadd_rn(__fmul_rn(ex2, ex2), __fmul_rn(ey2, ey2)) > th2) return 5;
    return low ? 7 : 6;
}

__global__ __launch_bounds__(256) void reconstruct_check_kernel(Args a)
{
    const int i = blockIdx.x * 256 + threadIdx.x, h = blockIdx.y;
    if (i >= a.N) return;
    const int nhyp = a.head[0], model = a.head[1];
    const int i1 = a.pairs[2 * i], i2 = a.pairs[2 * i + 1]; // checked before either becomes an address
    const bool ok = pair_ok(a, i1, i2);
    if (!ok && h == 0) *a.status = ORBFE_ERR_INVALID; // every lane that writes writes this value
    int code = 0;
    float cosp = 0.f;
    if (ok && h < nhyp && (model == 0 ? a.inl_h : a.inl_f)[i]) {
        float p[3];
        code = check_match(a.hyp + h * HYP_FLOATS, a.K4, a.keys1[i1].x, a.keys1[i1].y, a.keys2[i2].x, a.keys2[i2].y, a.th2, cosp, p);
    }
    a.codes[(size_t)h * a.N + i] = (uint8_t)code;
    a.cos[(size_t)h * a.N + i] = cosp;
}

// ---------------------------------------------------------------------------------------------------------------- the choice
// keys whose unsigned order is the sorted order of the cosines: the floats' own, -0 before +0, any NaN after every number
__device__ __forceinline__ unsigned order_key(float c)
{
    const unsigned b = __float_as_uint(c);
    if (c != c) return 0xFFFFFFFFu;
    return (b >> 31) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float key_value(unsigned key)
{
    if (key == 0xFFFFFFFFu) return __int_as_float(0x7fc00000);
    return __uint_as_float((key >> 31) ? (key & 0x7FFFFFFFu) : ~key);
}

__global__ __launch_bounds__(256) void reconstruct_select_kernel(Args a)
{
    __shared__ int s_hist[256];
    __shared__ int s_sel[2];   // selected digit, rank inside the digit's bucket
    __shared__ int s_count[9]; // nGood per hypothesis, then the number of set inlier flags
    __shared__ int s_choice;
    const int tid = threadIdx.x, lane = tid & 63;
    const int nhyp = a.head[0], model = a.head[1], early = a.head[2];
    const uint8_t *flags = model == 0 ? a.inl_h : a.inl_f;
    if (tid < 9) s_count[tid] = 0;
    __syncthreads();
    {
        int n = 0;
        for (int i = tid; i < a.N; i += 256) n += flags[i] != 0;
        if (n) atomicAdd(&s_count[8], n);
        for (int h = 0; h < nhyp; h++) {
            n = 0;
            for (int i = tid; i < a.N; i += 256) n += a.codes[(size_t)h * a.N + i] >= 6;
            if (n) atomicAdd(&s_count[h], n);
        }
    }
    __syncthreads();
    // vCosParallax[min(50, size - 1)] after the sort (:897-900): a radix select over the counted entries' keys, 8 bits a pass
    for (int h = 0; h < nhyp; h++) {
        const int total = s_count[h];
        if (total == 0) continue; // uniform
        const uint8_t *codes = a.codes + (size_t)h * a.N;
        const float *cosv = a.cos + (size_t)h * a.N;
        unsigned prefix = 0, mask = 0;
        if (tid == 0) s_sel[1] = total - 1 < 50 ? total - 1 : 50;
        for (int shift = 24; shift >= 0; shift -= 8) {
            s_hist[tid] = 0;
            __syncthreads();
            for (int i = tid; i < a.N; i += 256)
                if (codes[i] >= 6) {
                    const unsigned key = order_key(cosv[i]);
                    if ((key & mask) == prefix) atomicAdd(&s_hist[(key >> shift) & 255u], 1);
                }
            __syncthreads();
            if (tid < 64) { // the digit that holds the wanted rank: a lane owns 4 bins, a wave scan, the owner lane resolves its bins
                const int h0 = s_hist[4 * lane], h1 = s_hist[4 * lane + 1], h2 = s_hist[4 * lane + 2], h3 = s_hist[4 * lane + 3];
                const int sum = h0 + h1 + h2 + h3;
                int inc = sum;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int t = __shfl_up(inc, o, 64);
                    if (lane >= o) inc += t;
                }
                const int rank = s_sel[1], before = inc - sum;
                if (rank >= before && rank < inc) {
                    int r = rank - before, d = 4 * lane;
                    if (r >= h0) { r -= h0; d++; if (r >= h1) { r -= h1; d++; if (r >= h2) { r -= h2; d++; } } }
                    s_sel[0] = d;
                    s_sel[1] = r;
                }
            }
            __syncthreads();
            prefix |= (unsigned)s_sel[0] << shift;
            mask |= 255u << shift;
            __syncthreads();
        }
        if (tid == 0) a.cos_parallax[h] = key_value(prefix);
    }
    if (tid == 0) {
        for (int h = 0; h < 8; h++) {
            a.ngood[h] = s_count[h];
            if (s_count[h] == 0) a.cos_parallax[h] = 2.0f;
        }
        const int Ninl = s_count[8];
        int chosen = -1, result = early;
        if (!early) {
            if (model == 1) { // :498-566
                int maxGood = s_count[0];
                for (int h = 1; h < 4; h++) maxGood = s_count[h] > maxGood ? s_count[h] : maxGood;
                const int ninety = (int)(0.9 * Ninl), nMinGood = ninety > a.min_triangulated ? ninety : a.min_triangulated;
                int nsimilar = 0;
                for (int h = 0; h < 4; h++) nsimilar += (double)s_count[h] > 0.7 * maxGood;
                if (!(maxGood < nMinGood || nsimilar > 1))
                    for (int h = 3; h >= 0; h--)
                        if (s_count[h] == maxGood) chosen = h; // the else-if chain never looks past the first
            } else {          // :688-720
                int bestGood = 0, second = 0, idx = -1;
                for (int h = 0; h < 8; h++) {
                    const int n = s_count[h];
                    if (n > bestGood) { second = bestGood; bestGood = n; idx = h; }
                    else if (n > second) second = n;
                }
                if ((double)second < 0.75 * bestGood && bestGood > a.min_triangulated && (double)bestGood > 0.9 * Ninl) chosen = idx;
            }
            result = chosen >= 0 ? 0 : 3;
        }
        *a.result = result;
        *a.choice = chosen;
        s_choice = chosen;
    }
    for (int i = tid; i < a.n1; i += 256) {
        a.p3d[3 * (size_t)i] = 0.f; a.p3d[3 * (size_t)i + 1] = 0.f; a.p3d[3 * (size_t)i + 2] = 0.f;
        a.triangulated[i] = 0;
    }
    __syncthreads(); // the cleared entries are in place before a chosen point lands on one
    const int chosen = s_choice;
    if (chosen < 0) return;
    const float *rec = a.hyp + chosen * HYP_FLOATS;
    if (tid < 12) {
        const float v = one_nan(rec[tid]);
        if (tid < 9) a.R21[tid] = v;
        else a.t21[tid - 9] = v;
    }
    const uint8_t *codes = a.codes + (size_t)chosen * a.N;
    for (int i = tid; i < a.N; i += 256) {
        if (codes[i] < 6) continue;
        const int i1 = a.pairs[2 * i], i2 = a.pairs[2 * i + 1]; // a counted entry has passed pair_ok
        float cosp, p[3];
        const int code = check_match(rec, a.K4, a.keys1[i1].x, a.keys1[i1].y, a.keys2[i2].x, a.keys2[i2].y, a.th2, cosp, p);
        a.p3d[3 * (size_t)i1] = p[0]; a.p3d[3 * (size_t)i1 + 1] = p[1]; a.p3d[3 * (size_t)i1 + 2] = p[2];
        a.triangulated[i1] = code == 7;
    }
}

// ---------------------------------------------------------------------------------------------------------------- entry points
// what the values alone show, for both forms: 0, or the refusal
static int refuse_values(orbfe_context *ctx, int n1, int n2, int N, const float *K, float sigma, int min_triangulated, int model)
{
    if (N < 1) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "reconstruct_initial: N = %d < 1", N);
    if (n1 < 0 || n2 < 0) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "reconstruct_initial: negative count");
    if (N > ORBFE_INITIALIZER_MAX_MATCHES || n1 > ORBFE_INITIALIZER_MAX_KEYS || n2 > ORBFE_INITIALIZER_MAX_KEYS)
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "reconstruct_initial: a count above its limit (N %d, n1 %d, n2 %d)", N, n1, n2);
    if (!(sigma > 0)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "reconstruct_initial: sigma must be > 0");
    if (!(K[0] > 0) || !(K[1] > 0)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "reconstruct_initial: fx and fy must be > 0");
    if (min_triangulated < 0) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "reconstruct_initial: min_triangulated = %d < 0", min_triangulated);
    if (model < -1 || model > 1) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "reconstruct_initial: model = %d outside -1 .. 1", model);
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    return ORBFE_OK;
}

// ReconstructF / ReconstructH on the outputs of orbfe_enqueue_find_homography_fundamental: a memset and three launches.
extern "C" int orbfe_enqueue_reconstruct_initial(orbfe_context *ctx, const orbfe_keypoint *d_keys1_un, int n1, const orbfe_keypoint *d_keys2_un, int n2,
                                                 const int32_t *d_pairs, int N, const float *d_H21, const float *d_F21, const float *d_score,
                                                 const int32_t *d_best, const uint8_t *d_inliers_h, const uint8_t *d_inliers_f, const float *K, float sigma,
                                                 int min_triangulated, int model, int32_t *d_model, float *d_hyp_R, float *d_hyp_t, int32_t *d_ngood,
                                                 float *d_cos_parallax, int32_t *d_result, int32_t *d_choice, float *d_R21, float *d_t21, float *d_p3d,
                                                 uint8_t *d_triangulated, uint8_t *d_codes, int32_t *d_status, void *stream)
try {
    ORBFE_ENTRY(ctx);
    // what the arguments alone show is refused first, so that the refusals can be told apart without a device
    if (!d_keys1_un || !d_keys2_un || !d_pairs || !d_H21 || !d_F21 || !d_score || !d_best || !d_inliers_h || !d_inliers_f || !K)
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "reconstruct_initial: null input");
    if (!d_model || !d_hyp_R || !d_hyp_t || !d_ngood || !d_cos_parallax || !d_result || !d_choice || !d_R21 || !d_t21 || !d_p3d || !d_triangulated || !d_status)
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "reconstruct_initial: null output");
    if (const int rc = refuse_values(ctx, n1, n2, N, K, sigma, min_triangulated, model)) return rc;
    hipStream_t s;
    if (const int rc = orbfe_enqueue_on(ctx, stream, false, &s)) return rc;
    const size_t entries = 8 * (size_t)N, head_bytes = 16 + 8 * HYP_FLOATS * 4;
    if (ctx->recon_scratch.ensure(head_bytes + entries * 5) != 0) return orbfe_fail(ctx, ORBFE_ERR_HIP, "reconstruct_initial: scratch allocation failed");
    Args a;
    a.keys1 = d_keys1_un; a.keys2 = d_keys2_un; a.pairs = d_pairs; a.H21 = d_H21; a.F21 = d_F21; a.score = d_score; a.best = d_best;
    a.inl_h = d_inliers_h; a.inl_f = d_inliers_f;
    a.n1 = n1; a.n2 = n2; a.N = N; a.min_triangulated = min_triangulated; a.model = model;
    for (int k = 0; k < 4; k++) a.K4[k] = K[k];
    a.th2 = (float)(4.0 * (double)(sigma * sigma));
    a.out_model = d_model; a.hyp_R = d_hyp_R; a.hyp_t = d_hyp_t; a.ngood = d_ngood; a.cos_parallax = d_cos_parallax; a.result = d_result; a.choice = d_choice;
    a.R21 = d_R21; a.t21 = d_t21; a.p3d = d_p3d; a.triangulated = d_triangulated; a.status = d_status;
    a.head = (int32_t *)ctx->recon_scratch.p; a.hyp = (float *)(a.head + 4); a.cos = a.hyp + 8 * HYP_FLOATS;
    a.codes = d_codes ? d_codes : (uint8_t *)(a.cos + entries);
    ORBFE_HIP_TRY(ctx, hipMemsetAsync(a.status, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(reconstruct_hypotheses_kernel, dim3(1), dim3(64), 0, s, a);
    hipLaunchKernelGGL(reconstruct_check_kernel, dim3((N + 255) / 256, 8), dim3(256), 0, s, a);
    hipLaunchKernelGGL(reconstruct_select_kernel, dim3(1), dim3(256), 0, s, a);
    ORBFE_HIP_TRY(ctx, hipGetLastError());
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

extern "C" int orbfe_reconstruct_initial(orbfe_context *ctx, const orbfe_keypoint *keys1_un, int n1, const orbfe_keypoint *keys2_un, int n2, const int32_t *pairs,
                                         int N, const float *H21, const float *F21, const float *score, const int32_t *best, const uint8_t *inliers_h,
                                         const uint8_t *inliers_f, const float *K, float sigma, float min_parallax, int min_triangulated, int model,
                                         int32_t *out_model, float *hyp_R, float *hyp_t, int32_t *ngood, float *cos_parallax, int32_t *result, int32_t *choice,
                                         float *R21, float *t21, float *p3d, uint8_t *triangulated, uint8_t *codes, int *ok)
try {
    ORBFE_ENTRY(ctx);
    if (!keys1_un || !keys2_un || !pairs || !H21 || !F21 || !score || !best || !inliers_h || !inliers_f || !K)
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "reconstruct_initial: null input");
    if (!out_model || !hyp_R || !hyp_t || !ngood || !cos_parallax || !result || !choice || !R21 || !t21 || !p3d || !triangulated || !ok)
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "reconstruct_initial: null output");
    if (const int rc = refuse_values(ctx, n1, n2, N, K, sigma, min_triangulated, model)) return rc;
    hipStream_t s;
    if (const int rc = orbfe_enqueue_on(ctx, nullptr, false, &s)) return rc;
    // one device block: inputs, then outputs
    const size_t kb1 = sizeof(orbfe_keypoint) * (size_t)n1, kb2 = sizeof(orbfe_keypoint) * (size_t)n2, nn = (size_t)N;
    orbfe::Arena c(nullptr, 16, 0);
    const size_t o_k1 = c.take_bytes(1, kb1), o_k2 = c.take_bytes(1, kb2), o_pairs = c.take_bytes(8, nn), o_in = c.take_bytes(4, 24), o_ih = c.take_bytes(1, nn),
                 o_if = c.take_bytes(1, nn), o_small = c.take_bytes(4, 160), o_p3d = c.take_bytes(12, n1), o_tri = c.take_bytes(1, n1),
                 o_codes = c.take_bytes(8, codes ? nn : 0);
    if (ctx->sync_stage.ensure(c.bytes()) != 0) return orbfe_fail(ctx, ORBFE_ERR_HIP, "reconstruct_initial: device allocation failed");
    uint8_t *d = (uint8_t *)ctx->sync_stage.p;
    if (kb1) ORBFE_HIP_TRY(ctx, hipMemcpyAsync(d + o_k1, keys1_un, kb1, hipMemcpyHostToDevice, s));
    if (kb2) ORBFE_HIP_TRY(ctx, hipMemcpyAsync(d + o_k2, keys2_un, kb2, hipMemcpyHostToDevice, s));
    ORBFE_HIP_TRY(ctx, hipMemcpyAsync(d + o_pairs, pairs, 8 * nn, hipMemcpyHostToDevice, s));
    // small inputs: H21 [0, 9), F21 [9, 18), score [18, 20), best [20, 22)
    float in[24] = {};
    memcpy(in, H21, 36); memcpy(in + 9, F21, 36); memcpy(in + 18, score, 8); memcpy(in + 20, best, 8);
    ORBFE_HIP_TRY(ctx, hipMemcpyAsync(d + o_in, in, sizeof(in), hipMemcpyHostToDevice, s));
    ORBFE_HIP_TRY(ctx, hipMemcpyAsync(d + o_ih, inliers_h, nn, hipMemcpyHostToDevice, s));
    ORBFE_HIP_TRY(ctx, hipMemcpyAsync(d + o_if, inliers_f, nn, hipMemcpyHostToDevice, s));
    // small outputs: hyp_R [0, 72), hyp_t [72, 96), R21 [96, 105), t21 [105, 108), cos [108, 116), ngood [116, 124), model, result, choice, status [124, 128);
    // what the call may leave untouched starts as the caller's
    float small[160] = {};
    memcpy(small, hyp_R, 288); memcpy(small + 72, hyp_t, 96); memcpy(small + 96, R21, 36); memcpy(small + 105, t21, 12);
    ORBFE_HIP_TRY(ctx, hipMemcpyAsync(d + o_small, small, sizeof(small), hipMemcpyHostToDevice, s));
    float *di = (float *)(d + o_in), *ds = (float *)(d + o_small);
    const int rc = orbfe_enqueue_reconstruct_initial(ctx, (const orbfe_keypoint *)(d + o_k1), n1, (const orbfe_keypoint *)(d + o_k2), n2, (const int32_t *)(d + o_pairs), N,
                                                     di, di + 9, di + 18, (const int32_t *)(di + 20), d + o_ih, d + o_if, K, sigma, min_triangulated, model,
                                                     (int32_t *)(ds + 124), ds, ds + 72, (int32_t *)(ds + 116), ds + 108, (int32_t *)(ds + 125), (int32_t *)(ds + 126),
                                                     ds + 96, ds + 105, (float *)(d + o_p3d), d + o_tri, codes ? d + o_codes : nullptr, (int32_t *)(ds + 127), s);
    if (rc != ORBFE_OK) return rc;
    ORBFE_HIP_TRY(ctx, hipMemcpyAsync(small, d + o_small, sizeof(small), hipMemcpyDeviceToHost, s));
    if (n1) ORBFE_HIP_TRY(ctx, hipMemcpyAsync(p3d, d + o_p3d, 12 * (size_t)n1, hipMemcpyDeviceToHost, s));
    if (n1) ORBFE_HIP_TRY(ctx, hipMemcpyAsync(triangulated, d + o_tri, n1, hipMemcpyDeviceToHost, s));
    if (codes) ORBFE_HIP_TRY(ctx, hipMemcpyAsync(codes, d + o_codes, 8 * nn, hipMemcpyDeviceToHost, s));
    ORBFE_HIP_TRY(ctx, hipStreamSynchronize(s));
    memcpy(hyp_R, small, 288); memcpy(hyp_t, small + 72, 96); memcpy(R21, small + 96, 36); memcpy(t21, small + 105, 12);
    memcpy(cos_parallax, small + 108, 32); memcpy(ngood, small + 116, 32);
    int32_t tail[4];
    memcpy(tail, small + 124, 16);
    *out_model = tail[0]; *result = tail[1]; *choice = tail[2];
    // the parallax test (:524 / :720): the one comparison that stays on the host
    *ok = tail[1] == 0 && tail[2] >= 0 && tail[2] < 8 && ORB_SLAM2::ReconstructAccept(tail[0], cos_parallax[tail[2]], min_parallax) ? 1 : 0;
    if (tail[3] != 0) return orbfe_fail(ctx, tail[3], "reconstruct_initial: the device reported a faulty pair index");
    return ORBFE_OK;
} ORBFE_CATCH(ctx)
