// orbfe_initializer_device.hip -- Initializer::FindHomography and Initializer::FindFundamental (src/Initializer.cc:123-467) for one frame
// pair, every RANSAC hypothesis of both models, asynchronous on the caller's stream.  The entry points and their checks are at the
// end of this file; the arithmetic contract is stated in include/orbfe.h and DESIGN.md section 4l, and this file,
// orbslam2_amd/host/Initializer.h and tests/initializer_model.py follow it operation by operation.
//
//   initializer_models_kernel   one wave per (set, model).  The 9 x 16 At, the 9 x 9 Vt and W live in LDS (dynamic row indices in private
//                               arrays would go to scratch memory).  Every lane reads both rows of a pair whole (four b128 loads each, at a
//                               fixed 16 entries: zero rows change no bit) and evaluates the double dot product, c, s, both rotated rows and
//                               their square sums in index order -- the same values in all lanes, so the branches are uniform -- then
//                               lanes 0..15 write one element of At each, lanes 16..24 one of Vt: one LDS round trip per rotation.  The 3 x 3 steps (products, inverse, the rank-2 step's second
//                               Jacobi) follow in the same wave.  The wave leaves H21i, H12i / F21i in the context's scratch.
//   initializer_score_kernel    one lane per (hypothesis, model) adds its 2 N terms in match order: the score is a sequential float sum by
//                               definition, so a hypothesis is one dependent chain whatever computes the terms.  Lanes of a wave share the
//                               match, so its keypoints are loaded once per wave.
//   initializer_select_kernel   one workgroup per model: wave 0 takes the first strict maximum, then all 256 lanes evaluate the winner's
//                               inlier flags (the same float operations as the score kernel, so the same bits) and count them.
// All stores are plain vector stores.
#include "../../include/orbfe.h"
#include "orbfe_config.h"
#include "orbfe_host.h"
#include "../host/Initializer.h"
#include "orbfe_cvmat.hpp"
#include "orbfe_jacobi_wave.hpp"

#include <cfloat>

// what every kernel of this file takes.  T1, T2inv and T2t are made on the host from the two Normalize results; mats, ok and scores
// are the context's scratch.
struct orbfe_initializer_args {
    const orbfe_keypoint *keys1, *keys2;
    const int32_t *pairs, *sets;
    int n1, n2, N, iterations;
    float norm1[4], norm2[4], T1[9], T2inv[9], T2t[9], inv_sigma2;
    float *H21, *F21, *score;
    int32_t *best;
    uint8_t *inl_h, *inl_f;
    int32_t *ninliers;
    float *all_scores;
    int32_t *status;
    float *mats;     // [iterations][27]: H21i, H12i, F21i
    int32_t *ok;     // [iterations]: the set's eight matches are addressable
    float *scores;   // [2][iterations], as summed (a NaN keeps its bits here)
};
typedef orbfe_initializer_args Args;

static_assert(sizeof(orbfe_keypoint) == 28, "orbfe_keypoint");

__device__ __forceinline__ bool pair_ok(const Args &a, int i1, int i2) { return i1 >= 0 && i1 < a.n1 && i2 >= 0 && i2 < a.n2; }

// ---------------------------------------------------------------------------------------------------------------- the models
__global__ __launch_bounds__(64) void initializer_models_kernel(Args a)
{
    __shared__ __attribute__((aligned(16))) float At[9 * AT_STRIDE];
    __shared__ float Vt[9 * VT_STRIDE];
    __shared__ double W[9];
    const int it = blockIdx.x, model = blockIdx.y, lane = threadIdx.x;

    // Select a minimum set: lane j < 8 takes match mvSets[it][j]; every index is checked before it becomes an address
    bool ok = true;
    float u1 = 0.f, v1 = 0.f, u2 = 0.f, v2 = 0.f;
    if (lane < 8) {
        const int idx = a.sets[8 * (size_t)it + lane];
        ok = idx >= 0 && idx < a.N;
        if (ok) {
            const int i1 = a.pairs[2 * idx], i2 = a.pairs[2 * idx + 1];
            ok = pair_ok(a, i1, i2);
            if (ok) {
                u1 = __fmul_rn(__fsub_rn(a.keys1[i1].x, a.norm1[0]), a.norm1[2]); v1 = __fmul_rn(__fsub_rn(a.keys1[i1].y, a.norm1[1]), a.norm1[3]);
                u2 = __fmul_rn(__fsub_rn(a.keys2[i2].x, a.norm2[0]), a.norm2[2]); v2 = __fmul_rn(__fsub_rn(a.keys2[i2].y, a.norm2[1]), a.norm2[3]);
            }
        }
    }
    if (!__all(ok)) { // a faulty hypothesis is skipped: the score kernel gives it 0 and it never wins
        if (lane == 0) {
            if (model == 0) a.ok[it] = 0;
            *a.status = ORBFE_ERR_INVALID; // every lane that writes writes this value
        }
        return;
    }
    if (lane == 0 && model == 0) a.ok[it] = 1;

    for (int e = lane; e < 9 * AT_STRIDE; e += 64) At[e] = 0.f;
    __syncthreads();
    if (lane < 8) {
        if (model == 0) { // ComputeH21 (:238-256)
            const float r0[9] = {0.f, 0.f, 0.f, -u1, -v1, -1.f, __fmul_rn(v2, u1), __fmul_rn(v2, v1), v2};
            const float r1[9] = {u1, v1, 1.f, 0.f, 0.f, 0.f, __fmul_rn(-u2, u1), __fmul_rn(-u2, v1), -u2};
#pragma unroll
            for (int c = 0; c < 9; c++) { At[c * AT_STRIDE + 2 * lane] = r0[c]; At[c * AT_STRIDE + 2 * lane + 1] = r1[c]; }
        } else {          // ComputeF21 (:280-288); row 8 stays zero
            const float r[9] = {__fmul_rn(u2, u1), __fmul_rn(u2, v1), u2, __fmul_rn(v2, u1), __fmul_rn(v2, v1), v2, u1, v1, 1.f};
#pragma unroll
            for (int c = 0; c < 9; c++) At[c * AT_STRIDE + lane] = r[c];
        }
    }
    __syncthreads();
    jacobi_wave<9, 16>(At, Vt, W, lane); // F's rows 8 .. 15 are zero

    float X[9], t[9], M[9]; // vt.row(8).reshape(0, 3), in every lane
#pragma unroll
    for (int k = 0; k < 9; k++) X[k] = Vt[8 * VT_STRIDE + k];
    float *out = a.mats + (size_t)it * 27;
    if (model == 0) {
        mul3(a.T2inv, X, t);
        mul3(t, a.T1, M);      // H21i = T2inv * Hn * T1
        float Mi[9];
        inv3(M, Mi);           // H12i = H21i.inv()
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 9; k++) { out[k] = M[k]; out[9 + k] = Mi[k]; }
        }
        return;
    }
    // the rank-2 step (:297-301): the same Jacobi on the 3 x 3 Fpre; At row i = column i of Fpre
    __syncthreads();
    if (lane < 9) At[(lane / 3) * AT_STRIDE + lane % 3] = Vt[8 * VT_STRIDE + 3 * (lane % 3) + lane / 3];
    if (lane < 3) At[lane * AT_STRIDE + 3] = 0.f; // the fourth, zero row of the 3 x 3 problem
    __syncthreads(); // jacobi_wave's first step overwrites Vt only after its own reads of At; the read of Vt above is complete here
    jacobi_wave<3, 4>(At, Vt, W, lane);
    float u[9], d[9], vt[9];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double w = W[i];
        const float s = w > (double)FLT_MIN ? (float)(1 / w) : 0.f; // the basis completion of a zero singular value is not restated
#pragma unroll
        for (int k = 0; k < 3; k++) {
            u[3 * k + i] = __fmul_rn(At[i * AT_STRIDE + k], s);
            vt[3 * i + k] = Vt[i * VT_STRIDE + k];
            d[3 * i + k] = 0.f;
        }
    }
    d[0] = (float)W[0]; d[4] = (float)W[1]; // w.at<float>(2) = 0
    mul3(u, d, t);
    mul3(t, vt, X);            // Fn = u * diag(w) * vt
    mul3(a.T2t, X, t);
    mul3(t, a.T1, M);          // F21i = T2t * Fn * T1
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 9; k++) out[18 + k] = M[k];
    }
}

// ---------------------------------------------------------------------------------------------------------------- the scores
// the two terms of one match in CheckHomography (:336-384): returns bIn, adds to the running float sum
__device__ __forceinline__ bool score_h(const float (&H)[18], float u1, float v1, float u2, float v2, float inv_sigma2, float &score)
{
    const float th = 5.991f;
    bool in = true;
    const float w2 = (float)(1.0 / (double)__fadd_rn(__fadd_rn(__fmul_rn(H[15], u2), __fmul_rn(H[16], v2)), H[17]));
    const float u2in1 = __fmul_rn(__fadd_rn(__fadd_rn(__fmul_rn(H[9], u2), __fmul_rn(H[10], v2)), H[11]), w2);
    const float v2in1 = __fmul_rn(__fadd_rn(__fadd_rn(__fmul_rn(H[12], u2), __fmul_rn(H[13], v2)), H[14]), w2);
    const float du1 = __fsub_rn(u1, u2in1), dv1 = __fsub_rn(v1, v2in1);
    const float chi1 = __fmul_rn(__fadd_rn(__fmul_rn(du1, du1), __fmul_rn(dv1, dv1)), inv_sigma2);
    if (chi1 > th) in = false;
    else score = __fadd_rn(score, __fsub_rn(th, chi1));
    const float w1 = (float)(1.0 / (double)__fadd_rn(__fadd_rn(__fmul_rn(H[6], u1), __fmul_rn(H[7], v1)), H[8]));
    const float u1in2 = __fmul_rn(__fadd_rn(__fadd_rn(__fmul_rn(H[0], u1), __fmul_rn(H[1], v1)), H[2]), w1);
    const float v1in2 = __fmul_rn(__fadd_rn(__fadd_rn(__fmul_rn(H[3], u1), __fmul_rn(H[4], v1)), H[5]), w1);
    const float du2 = __fsub_rn(u2, u1in2), dv2 = __fsub_rn(v2, v1in2);
    const float chi2 = __fmul_rn(__fadd_rn(__fmul_rn(du2, du2), __fmul_rn(dv2, dv2)), inv_sigma2);
    if (chi2 > th) in = false;
    else score = __fadd_rn(score, __fsub_rn(th, chi2));
    return in;
}

// the same of CheckFundamental (:412-464)
__device__ __forceinline__ bool score_f(const float (&F)[18], float u1, float v1, float u2, float v2, float inv_sigma2, float &score)
{
    const float th = 3.841f, th_score = 5.991f;
    bool in = true;
    const float a2 = __fadd_rn(__fadd_rn(__fmul_rn(F[0], u1), __fmul_rn(F[1], v1)), F[2]);
    const float b2 = __fadd_rn(__fadd_rn(__fmul_rn(F[3], u1), __fmul_rn(F[4], v1)), F[5]);
    const float c2 = __fadd_rn(__fadd_rn(__fmul_rn(F[6], u1), __fmul_rn(F[7], v1)), F[8]);
    const float num2 = __fadd_rn(__fadd_rn(__fmul_rn(a2, u2), __fmul_rn(b2, v2)), c2);
    const float chi1 = __fmul_rn(__fdiv_rn(__fmul_rn(num2, num2), __fadd_rn(__fmul_rn(a2, a2), __fmul_rn(b2, b2))), inv_sigma2);
    if (chi1 > th) in = false;
    else score = __fadd_rn(score, __fsub_rn(th_score, chi1));
    const float a1 = __fadd_rn(__fadd_rn(__fmul_rn(F[0], u2), __fmul_rn(F[3], v2)), F[6]);
    const float b1 = __fadd_rn(__fadd_rn(__fmul_rn(F[1], u2), __fmul_rn(F[4], v2)), F[7]);
    const float c1 = __fadd_rn(__fadd_rn(__fmul_rn(F[2], u2), __fmul_rn(F[5], v2)), F[8]);
    const float num1 = __fadd_rn(__fadd_rn(__fmul_rn(a1, u1), __fmul_rn(b1, v1)), c1);
    const float chi2 = __fmul_rn(__fdiv_rn(__fmul_rn(num1, num1), __fadd_rn(__fmul_rn(a1, a1), __fmul_rn(b1, b1))), inv_sigma2);
    if (chi2 > th) in = false;
    else score = __fadd_rn(score, __fsub_rn(th_score, chi2));
    return in;
}

// the matrices of hypothesis `it` for `model`: H21i, H12i or F21i (the second nine unused)
__device__ __forceinline__ void load_mats(const float *mats, int it, int model, float (&M)[18])
{
    const float *src = mats + (size_t)it * 27 + (model ? 18 : 0);
#pragma unroll
    for (int k = 0; k < 18; k++) M[k] = (model == 0 || k < 9) ? src[k] : 0.f;
}

__global__ __launch_bounds__(64) void initializer_score_kernel(Args a)
{
    const int it = blockIdx.x * 64 + threadIdx.x, model = blockIdx.y;
    if (it >= a.iterations) return;
    float score = 0.f;
    if (a.ok[it]) {
        float M[18];
        load_mats(a.mats, it, model, M);
        for (int i = 0; i < a.N; i++) {
            const int i1 = a.pairs[2 * i], i2 = a.pairs[2 * i + 1];
            if (!pair_ok(a, i1, i2)) continue; // a faulty match adds nothing; the select kernel reports it
            const float u1 = a.keys1[i1].x, v1 = a.keys1[i1].y, u2 = a.keys2[i2].x, v2 = a.keys2[i2].y;
            if (model == 0) score_h(M, u1, v1, u2, v2, a.inv_sigma2, score);
            else score_f(M, u1, v1, u2, v2, a.inv_sigma2, score);
        }
    }
    a.scores[(size_t)model * a.iterations + it] = score;
}

// ---------------------------------------------------------------------------------------------------------------- the winner
__global__ __launch_bounds__(256) void initializer_select_kernel(Args a)
{
    __shared__ int s_best, s_count;
    __shared__ float s_M[18];
    const int tid = threadIdx.x, model = blockIdx.x;
    const float *scores = a.scores + (size_t)model * a.iterations;
    if (tid < 64) {
        // `currentScore > score` from score = 0 in iteration order (:164, :215) ends at the first occurrence of the largest score above 0;
        // a NaN score compares false both ways.  Each lane scans its iterations in ascending order, then the lanes are merged.
        float bs = 0.f;
        int bi = -1;
        for (int it = tid; it < a.iterations; it += 64) {
            const float s = scores[it];
            if (s > bs) { bs = s; bi = it; }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float os = __shfl_xor(bs, off);
            const int oi = __shfl_xor(bi, off);
            if (oi >= 0 && (os > bs || (os == bs && (bi < 0 || oi < bi)))) { bs = os; bi = oi; }
        }
        if (tid == 0) {
            s_best = bi; s_count = 0;
            a.best[model] = bi;
            a.score[model] = bi >= 0 ? bs : 0.f;
        }
    }
    if (a.all_scores)
        for (int it = tid; it < a.iterations; it += 256) {
            const float s = scores[it];
            a.all_scores[(size_t)model * a.iterations + it] = s != s ? __int_as_float(0x7fc00000) : s; // one bit pattern for NaN
        }
    __syncthreads();
    const int best = s_best;
    if (best >= 0 && tid < (model == 0 ? 18 : 9)) {
        const float v = a.mats[(size_t)best * 27 + (model ? 18 : 0) + tid];
        s_M[tid] = v;
        if (tid < 9) (model == 0 ? a.H21 : a.F21)[tid] = v;
    }
    __syncthreads();
    float M[18];
#pragma unroll
    for (int k = 0; k < 18; k++) M[k] = (best >= 0 && (model == 0 || k < 9)) ? s_M[k] : 0.f;
    uint8_t *inl = model == 0 ? a.inl_h : a.inl_f;
    int count = 0;
    bool faulty = false;
    for (int i = tid; i < a.N; i += 256) {
        const int i1 = a.pairs[2 * i], i2 = a.pairs[2 * i + 1];
        bool in = false;
        if (!pair_ok(a, i1, i2)) faulty = true;
        else if (best >= 0) {
            const float u1 = a.keys1[i1].x, v1 = a.keys1[i1].y, u2 = a.keys2[i2].x, v2 = a.keys2[i2].y;
            float unused = 0.f;
            in = model == 0 ? score_h(M, u1, v1, u2, v2, a.inv_sigma2, unused) : score_f(M, u1, v1, u2, v2, a.inv_sigma2, unused);
        }
        if (inl) inl[i] = in ? 1 : 0;
        count += in;
    }
    if (faulty) *a.status = ORBFE_ERR_INVALID; // every lane that writes writes this value
    if (count) atomicAdd(&s_count, count);
    __syncthreads();
    if (tid == 0 && a.ninliers) a.ninliers[model] = s_count;
}

// Initializer::FindHomography + FindFundamental for one frame pair: a memset and three launches.
extern "C" int orbfe_enqueue_find_homography_fundamental(orbfe_context *ctx, const orbfe_keypoint *d_keys1_un, int n1, const orbfe_keypoint *d_keys2_un,
                                                         int n2, const int32_t *d_pairs, int N, const int32_t *d_sets, int iterations, const float *norm1,
                                                         const float *norm2, float sigma, float *d_H21, float *d_F21, float *d_score, int32_t *d_best,
                                                         uint8_t *d_inliers_h, uint8_t *d_inliers_f, int32_t *d_ninliers, float *d_all_scores,
                                                         int32_t *d_status, void *stream)
try {
    ORBFE_ENTRY(ctx);
    // what the arguments alone show is refused first, so that the refusals can be told apart without a device
    if (!d_keys1_un || !d_keys2_un || !d_pairs || !d_sets || !norm1 || !norm2) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "find_homography_fundamental: null input");
    if (!d_H21 || !d_F21 || !d_score || !d_best || !d_status) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "find_homography_fundamental: null output");
    if (N < 8) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "find_homography_fundamental: N = %d < 8", N);
    if (iterations < 1) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "find_homography_fundamental: iterations = %d < 1", iterations);
    if (n1 < 0 || n2 < 0) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "find_homography_fundamental: negative count");
    if (N > ORBFE_INITIALIZER_MAX_MATCHES || iterations > ORBFE_INITIALIZER_MAX_ITERATIONS || n1 > ORBFE_INITIALIZER_MAX_KEYS || n2 > ORBFE_INITIALIZER_MAX_KEYS)
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "find_homography_fundamental: a count above its limit (N %d, iterations %d, n1 %d, n2 %d)", N, iterations, n1, n2);
    if (!(sigma > 0)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "find_homography_fundamental: sigma must be > 0");
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    hipStream_t s;
    if (const int rc = orbfe_enqueue_on(ctx, stream, false, &s)) return rc;
    const size_t it = (size_t)iterations;
    if (ctx->init_scratch.ensure(it * (27 + 1 + 2) * 4) != 0) return orbfe_fail(ctx, ORBFE_ERR_HIP, "find_homography_fundamental: scratch allocation failed");
    Args a;
    a.keys1 = d_keys1_un; a.keys2 = d_keys2_un; a.pairs = d_pairs; a.sets = d_sets;
    a.n1 = n1; a.n2 = n2; a.N = N; a.iterations = iterations;
    float T2[9];
    for (int k = 0; k < 4; k++) { a.norm1[k] = norm1[k]; a.norm2[k] = norm2[k]; }
    ORB_SLAM2::InitializerT(a.norm1, a.T1);
    ORB_SLAM2::InitializerT(a.norm2, T2);
    ORB_SLAM2::Inv3(T2, a.T2inv);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) a.T2t[3 * r + c] = T2[3 * c + r];
    a.inv_sigma2 = (float)(1.0 / (double)(sigma * sigma));
    a.H21 = d_H21; a.F21 = d_F21; a.score = d_score; a.best = d_best; a.inl_h = d_inliers_h; a.inl_f = d_inliers_f; a.ninliers = d_ninliers;
    a.all_scores = d_all_scores; a.status = d_status;
    a.mats = (float *)ctx->init_scratch.p; a.ok = (int32_t *)(a.mats + it * 27); a.scores = (float *)(a.ok + it);
    ORBFE_HIP_TRY(ctx, hipMemsetAsync(a.status, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(initializer_models_kernel, dim3(a.iterations, 2), dim3(64), 0, s, a);
    hipLaunchKernelGGL(initializer_score_kernel, dim3((a.iterations + 63) / 64, 2), dim3(64), 0, s, a);
    hipLaunchKernelGGL(initializer_select_kernel, dim3(2), dim3(256), 0, s, a);
    ORBFE_HIP_TRY(ctx, hipGetLastError());
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

extern "C" int orbfe_find_homography_fundamental(orbfe_context *ctx, const orbfe_keypoint *keys1_un, int n1, const orbfe_keypoint *keys2_un, int n2,
                                                 const int32_t *matches12, const int32_t *sets, int iterations, float sigma, float *H21, float *F21,
                                                 float *score, int32_t *best, uint8_t *inliers_h, uint8_t *inliers_f, int32_t *ninliers, float *all_scores,
                                                 int32_t *n_matches)
try {
    ORBFE_ENTRY(ctx);
    if (!keys1_un || !keys2_un || !matches12 || !sets) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "find_homography_fundamental: null input");
    if (!H21 || !F21 || !score || !best || !n_matches) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "find_homography_fundamental: null output");
    if (n1 < 0 || n2 < 0 || n1 > ORBFE_INITIALIZER_MAX_KEYS || n2 > ORBFE_INITIALIZER_MAX_KEYS || iterations < 1 || iterations > ORBFE_INITIALIZER_MAX_ITERATIONS)
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "find_homography_fundamental: a count outside its range (iterations %d, n1 %d, n2 %d)", iterations, n1, n2);
    std::vector<int32_t> pairs; // mvMatches12 (:50-62)
    pairs.reserve(2 * (size_t)n1);
    for (int i = 0; i < n1; i++)
        if (matches12[i] >= 0) { pairs.push_back(i); pairs.push_back(matches12[i]); }
    const int N = (int)(pairs.size() / 2);
    *n_matches = N;
    if (N < 8) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "find_homography_fundamental: N = %d < 8", N);
    if (N > ORBFE_INITIALIZER_MAX_MATCHES) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "find_homography_fundamental: N = %d above its limit", N);
    if (!(sigma > 0)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "find_homography_fundamental: sigma must be > 0");
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    float norm1[4], norm2[4];
    ORB_SLAM2::NormalizeKeys(keys1_un, n1, norm1);
    ORB_SLAM2::NormalizeKeys(keys2_un, n2, norm2);
    hipStream_t s;
    if (const int rc = orbfe_enqueue_on(ctx, nullptr, false, &s)) return rc;
    // one device block: inputs, then outputs
    const size_t it = (size_t)iterations, kb1 = sizeof(orbfe_keypoint) * (size_t)n1, kb2 = sizeof(orbfe_keypoint) * (size_t)n2;
    orbfe::Arena c(nullptr, 16, 0);
    const size_t o_k1 = c.take_bytes(1, kb1), o_k2 = c.take_bytes(1, kb2), o_pairs = c.take_bytes(8, N), o_sets = c.take_bytes(32, it), o_small = c.take_bytes(4, 32),
                 o_ih = c.take_bytes(1, N), o_if = c.take_bytes(1, N), o_all = c.take_bytes(8, it);
    if (ctx->sync_stage.ensure(c.bytes()) != 0) return orbfe_fail(ctx, ORBFE_ERR_HIP, "find_homography_fundamental: device allocation failed");
    uint8_t *d = (uint8_t *)ctx->sync_stage.p;
    if (kb1) ORBFE_HIP_TRY(ctx, hipMemcpyAsync(d + o_k1, keys1_un, kb1, hipMemcpyHostToDevice, s));
    if (kb2) ORBFE_HIP_TRY(ctx, hipMemcpyAsync(d + o_k2, keys2_un, kb2, hipMemcpyHostToDevice, s));
    ORBFE_HIP_TRY(ctx, hipMemcpyAsync(d + o_pairs, pairs.data(), 8 * (size_t)N, hipMemcpyHostToDevice, s));
    ORBFE_HIP_TRY(ctx, hipMemcpyAsync(d + o_sets, sets, 32 * it, hipMemcpyHostToDevice, s));
    // small outputs: H21 [0, 9), F21 [9, 18), score [18, 20), best [20, 22), ninliers [22, 24), status [24]; they start as the caller's H21 / F21
    float small[32] = {};
    memcpy(small, H21, 36); memcpy(small + 9, F21, 36);
    ORBFE_HIP_TRY(ctx, hipMemcpyAsync(d + o_small, small, sizeof(small), hipMemcpyHostToDevice, s));
    float *ds = (float *)(d + o_small);
    const int rc = orbfe_enqueue_find_homography_fundamental(ctx, (const orbfe_keypoint *)(d + o_k1), n1, (const orbfe_keypoint *)(d + o_k2), n2,
                                                             (const int32_t *)(d + o_pairs), N, (const int32_t *)(d + o_sets), iterations, norm1, norm2, sigma, ds,
                                                             ds + 9, ds + 18, (int32_t *)(ds + 20), d + o_ih, d + o_if, (int32_t *)(ds + 22), (float *)(d + o_all),
                                                             (int32_t *)(ds + 24), s);
    if (rc != ORBFE_OK) return rc;
    ORBFE_HIP_TRY(ctx, hipMemcpyAsync(small, d + o_small, sizeof(small), hipMemcpyDeviceToHost, s));
    if (inliers_h) ORBFE_HIP_TRY(ctx, hipMemcpyAsync(inliers_h, d + o_ih, N, hipMemcpyDeviceToHost, s));
    if (inliers_f) ORBFE_HIP_TRY(ctx, hipMemcpyAsync(inliers_f, d + o_if, N, hipMemcpyDeviceToHost, s));
    if (all_scores) ORBFE_HIP_TRY(ctx, hipMemcpyAsync(all_scores, d + o_all, 8 * it, hipMemcpyDeviceToHost, s));
    ORBFE_HIP_TRY(ctx, hipStreamSynchronize(s));
    memcpy(H21, small, 36); memcpy(F21, small + 9, 36); memcpy(score, small + 18, 8); memcpy(best, small + 20, 8);
    if (ninliers) memcpy(ninliers, small + 22, 8);
    int32_t status;
    memcpy(&status, small + 24, 4);
    if (status != 0) return orbfe_fail(ctx, status, "find_homography_fundamental: the device reported a faulty pair or set index");
    return ORBFE_OK;
} ORBFE_CATCH(ctx)
