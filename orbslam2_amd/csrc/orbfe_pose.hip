// orbfe_pose.hip -- Optimizer::PoseOptimization (src/Optimizer.cc:283-495) on the device: the motion-only bundle
// adjustment that follows every Tracking matcher call (src/Tracking.cc:875,998,1040,1475,1555,1580).
//
// One workgroup per frame (problem).  The reference drives g2o's Levenberg solver over one 6-dof vertex and <= N unary
// edges; everything per-edge (projection, Huber weight, J^T W J, J^T W e, robust chi2) is data parallel, everything per
// trial step (6x6 LDLT with diagonal pivoting, SE3 exponential, acceptance test) is a few hundred flops that every
// lane repeats redundantly so that no broadcast is needed.  One evaluation pass produces the robust chi2 AND the
// normal equations at the trial pose: when the trial is accepted they are exactly what the next iteration's
// computeActiveErrors + buildSystem would produce (same pose, same edges), so an iteration costs one pass and one
// barrier.  All arithmetic is FP64 like g2o's; the block reduction has a fixed order (bit-reproducible run to run),
// which differs from the reference's edge-sequential sums, so the result agrees with the CPU to rounding
// (tests/test_pose.py states the tolerance).
//
// g2o call map:  eval_pass            = SparseOptimizer::computeActiveErrors + activeRobustChi2
//                                       (core/sparse_optimizer.cpp:61-114) + BlockSolver::buildSystem
//                                       (core/block_solver.hpp:502-560) with BaseUnaryEdge::constructQuadraticForm
//                                       (core/base_unary_edge.hpp:45-72) and the analytic Jacobians
//                                       (types/types_six_dof_expmap.cpp:266-288,335-364)
//                solve_ldlt6          = LinearSolverDense::solve (solvers/linear_solver_dense.h:65-112, Eigen::LDLT)
//                se3_exp / se3_mul    = SE3Quat::exp, operator* (types/se3quat.h:103-109,218-252)
//                the do/while         = OptimizationAlgorithmLevenberg::solve
//                                       (core/optimization_algorithm_levenberg.cpp:59-157)
// eval_pass, solve_ldlt6 and the SE3 algebra are in orbfe_pose_blocks.hpp, where tests/pose_blocks/pose_blocks.hip can run them
// one at a time (tests/test_pose_blocks.py); this file keeps the kernel and the host entry points.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cfloat>
#include <cstdint>
#include <cstring>

#include "orbfe_device.h"
#include "orbfe_host.h"

#include "orbfe_pose_blocks.hpp" // Se3 ... solve_ldlt6 ... eval_pass, and this stage's fp contract(fast) pragma

// (stated again so that pose_opt_kernel's contraction does not hang on what a header left in force)
#pragma clang fp contract(fast)

namespace {

constexpr int PO_THREADS = 256; // one wave per SIMD (512 threads measured slower: every wave repeats the per-trial serial part)

template <int THREADS, bool IN_LDS>
__global__ __launch_bounds__(THREADS) void pose_opt_kernel(const int32_t *__restrict__ offsets, const KeyPointPOD *__restrict__ keys,
                                                            const float *__restrict__ u_right, const uint8_t *__restrict__ has_point,
                                                            const float *__restrict__ Xw, float *__restrict__ Tcw,
                                                            uint8_t *__restrict__ outlier, int32_t *__restrict__ n_inliers,
                                                            const float *__restrict__ inv_sigma2, float fx, float fy, float cx,
                                                            float cy, float bf, int lds_cap)
{
    extern __shared__ double s_dyn[];
    double *s_rows = s_dyn;                         // [2][THREADS/16][32]  (double-buffered across passes)
    double *s_tot = s_rows + 2 * (THREADS / 16) * 32; // [2][32]
    __shared__ int s_cnt[2];
    const int prob = blockIdx.x;
    const int o0 = offsets[prob];
    EdgeTable E;
    E.n = offsets[prob + 1] - o0;
    E.keys = keys + o0; E.u_right = u_right + o0; E.has_point = has_point + o0; E.Xw = Xw + (size_t)3 * o0; E.outlier = outlier + o0;
    E.inv_sigma2 = inv_sigma2;
    E.cap = lds_cap;
    E.l_f = (float *)(s_tot + 2 * 32);
    E.l_st = (uint8_t *)(E.l_f + 7 * (size_t)lds_cap);
    float *T = Tcw + (size_t)16 * prob;
    const CamD cam = {(double)fx, (double)fy, (double)cx, (double)cy, (double)bf};
    const double delta_mono = (double)(float)sqrt(5.991), delta_stereo = (double)(float)sqrt(7.815); // src/Optimizer.cc:317-318
    const float chi2_mono = 5.991f, chi2_stereo = 7.815f;                                               // :408-409

    // edges start as inliers (:331,362)
    for (int i = threadIdx.x; i < E.n; i += THREADS) {
        const bool has = E.has_point[i] != 0;
        if constexpr (IN_LDS) {
            const KeyPointPOD kp = E.keys[i];
            E.l_f[0 * E.cap + i] = E.Xw[3 * (size_t)i];
            E.l_f[1 * E.cap + i] = E.Xw[3 * (size_t)i + 1];
            E.l_f[2 * E.cap + i] = E.Xw[3 * (size_t)i + 2];
            E.l_f[3 * E.cap + i] = kp.x;
            E.l_f[4 * E.cap + i] = kp.y;
            E.l_f[5 * E.cap + i] = E.u_right[i];
            E.l_f[6 * E.cap + i] = has ? inv_sigma2[kp.octave] : 0.f;
            E.l_st[i] = has ? 1 : 0;
        } else if (has) E.outlier[i] = 0;
    }
    // (each lane only ever touches the slots i = lane + k * THREADS: no barrier needed for the table itself)

    float Tin[16];
#pragma unroll
    for (int k = 0; k < 16; k++) Tin[k] = T[k];

    // s_tot[cur] holds the normal equations of the accepted estimate, s_tot[cur ^ 1] receives the trial's; s_rows toggles
    // every pass so that a fast wave's next pass cannot overwrite partials a slow wave still sums
    int rbuf = 0, cur = 0;
    double chi_s, cnt_s;
    double x[6] = {0, 0, 0, 0, 0, 0};
    Se3 est = se3_from_cv(Tin), last_eval = est;
    int ne = 0, n_bad = 0;
    bool robust = true;
#define PO_EVAL(pose, which)                                                                                                               \
    do {                                                                                                                                   \
        eval_pass<THREADS, IN_LDS>(E, pose, cam, robust, delta_mono, delta_stereo, s_rows + rbuf * (THREADS / 16) * 32, s_tot + (which) * 32, \
                                   chi_s, cnt_s);                                                                                          \
        rbuf ^= 1;                                                                                                                         \
    } while (0)
    for (int round = 0; round < 4; round++) {
        est = se3_from_cv(Tin); // :398
        PO_EVAL(est, cur);
        if (round == 0) {
            ne = (int)cnt_s;
            if (ne < 3) break; // :404-405
        }
        if (cnt_s > 0.0) { // otherwise optimize() returns before doing anything (no active vertex)
            last_eval = est;
            double current_chi = chi_s;
            double lambda = -1.0, ni = 2.0;
            int lm_bad = 0;
            for (int it = 0; it < 10; it++) {
                last_eval = est; // computeActiveErrors at the current estimate
                const double ini_chi = current_chi;
                const double *Hb = s_tot + cur * 32;
                if (it == 0) {
                    const double dg[6] = {Hb[0], Hb[6], Hb[11], Hb[15], Hb[18], Hb[20]};
                    double mx = 0.0;
#pragma unroll
                    for (int j = 0; j < 6; j++) mx = fmax(fabs(dg[j]), mx);
                    lambda = 1e-5 * mx;
                    ni = 2.0;
                    lm_bad = 0;
                }
                double rho = 0.0;
                int qmax = 0;
                do {
                    PO_T(t_s0);
                    const bool ok2 = solve_ldlt6(Hb, lambda, x);
                    PO_T(t_s1);
                    PO_ACC(0, t_s0, t_s1);
                    double scale = 0.0; // computeScale(), with the b of the system that produced x
#pragma unroll
                    for (int j = 0; j < 6; j++) scale += x[j] * (lambda * x[j] + Hb[21 + j]);
                    scale += 1e-3;
                    const Se3 trial = se3_mul(se3_exp(x), est);
                    PO_T(t_s2);
                    PO_ACC(1, t_s1, t_s2);
                    PO_EVAL(trial, cur ^ 1);
                    last_eval = trial;
                    const double temp_chi = ok2 ? chi_s : DBL_MAX;
                    rho = (current_chi - temp_chi) / scale;
                    if (rho > 0 && isfinite(temp_chi)) {
                        const double r21 = 2 * rho - 1;
                        double alpha = 1.0 - r21 * r21 * r21; // pow(2*rho-1, 3)
                        alpha = fmin(alpha, 2.0 / 3.0);
                        lambda *= fmax(1.0 / 3.0, alpha);
                        ni = 2;
                        current_chi = temp_chi;
                        est = trial;
                        cur ^= 1;
                        Hb = s_tot + cur * 32;
                    } else {
                        lambda *= ni;
                        ni *= 2;
                    }
                    qmax++;
                } while (rho < 0 && qmax < 10);
                if (qmax == 10 || rho == 0) break;
                if ((ini_chi - current_chi) * 1e3 < ini_chi) lm_bad++;
                else lm_bad = 0;
                if (lm_bad >= 3) break;
            }
        }
        // classification (:401-455); inliers keep the error of the last evaluated pose (Q11), outliers are recomputed
        int bad = 0;
        for (int i = threadIdx.x; i < E.n; i += THREADS) {
            const int st = edge_state<IN_LDS>(E, i);
            if (st == 0) continue;
            double Xw3[3], obs[3], info, err[3], p[3];
            bool stereo;
            edge_load<IN_LDS>(E, i, Xw3, obs, stereo, info);
            const float chi2 = (float)edge_error(st == 2 ? est : last_eval, cam, Xw3, obs, stereo, info, err, p);
            const bool out = chi2 > (stereo ? chi2_stereo : chi2_mono);
            edge_set_outlier<IN_LDS>(E, i, out);
            bad += out;
        }
        if (threadIdx.x == 0) s_cnt[round & 1] = 0;
        __syncthreads();
        for (int off = 32; off >= 1; off >>= 1) bad += __shfl_xor(bad, off, 64);
        if ((threadIdx.x & 63) == 0 && bad) atomicAdd(&s_cnt[round & 1], bad);
        __syncthreads();
        n_bad = s_cnt[round & 1];
        if (round == 2) robust = false; // :429-430
        if (ne < 10) break;             // :457-458
    }
#undef PO_EVAL
    if constexpr (IN_LDS) { // pFrame->mvbOutlier: written where a map point exists (cleared at edge creation even when ne < 3)
        for (int i = threadIdx.x; i < E.n; i += THREADS) {
            const int st = E.l_st[i];
            if (st) E.outlier[i] = st == 2 ? 1 : 0;
        }
    }
    if (threadIdx.x == 0) {
        if (ne >= 3) {
            float Tout[16];
            se3_to_cv(est, Tout);
#pragma unroll
            for (int k = 0; k < 16; k++) T[k] = Tout[k];
            n_inliers[prob] = ne - n_bad;
        } else n_inliers[prob] = 0;
    }
}

} // namespace

struct orbfe_pose_state {
    DevBuf blk, sig;          // one device block for all arrays of a host call
    uint8_t *h_blk = nullptr; // its pinned host image: one copy up, one copy down
    size_t h_bytes = 0;
};

orbfe_pose_state *orbfe_pose_state_create() { return new orbfe_pose_state(); }
void orbfe_pose_state_destroy(orbfe_pose_state *s)
{
    if (s && s->h_blk) (void)hipHostFree(s->h_blk);
    delete s;
}


extern "C" int orbfe_enqueue_pose_optimization(orbfe_context *ctx, int n_problems, const int32_t *d_offsets,
                                               const orbfe_keypoint *d_keys_un, const float *d_u_right, const uint8_t *d_has_point,
                                               const float *d_Xw, float *d_Tcw, uint8_t *d_outlier, int32_t *d_n_inliers,
                                               int max_keypoints, void *stream)
try {
    ORBFE_ENTRY(ctx);
    if (!ctx || n_problems < 0) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "bad argument");
    if (n_problems == 0) return ORBFE_OK;
    if (!d_offsets || !d_keys_un || !d_u_right || !d_has_point || !d_Xw || !d_Tcw || !d_outlier || !d_n_inliers)
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null device pointer");
    orbfe_pose_state *st = orbfe_ctx_pose_state(ctx);
    const orbfe_params *p = &ctx->params;
    hipStream_t s;
    if (const int rc = orbfe_enqueue_on(ctx, stream, false, &s)) return rc;
    if (!st->sig.p) { // mvInvLevelSigma2 of the context's pyramid
        if (st->sig.ensure(sizeof(float) * ORBFE_MAX_LEVELS)) return orbfe_fail(ctx, ORBFE_ERR_HIP, "pose scratch allocation failed");
        ORBFE_HIP_TRY(ctx, hipMemcpy(st->sig.p, ctx->plan.inv_sigma2, sizeof(float) * p->nlevels, hipMemcpyHostToDevice));
    }
    constexpr int TH = PO_THREADS;
    if (max_keypoints <= PO_LDS_CAP_MAX) {
        const int cap = (std::max(max_keypoints, 1) + 3) & ~3;
        const size_t lds = pose_lds_bytes<TH>(cap);
        static bool attr_set[64] = {}; // the attribute is per device
        const int dev = ctx->params.device;
        if (dev >= 0 && dev < 64 && !attr_set[dev]) {
            ORBFE_HIP_TRY(ctx, hipFuncSetAttribute((const void *)pose_opt_kernel<TH, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pose_lds_bytes<TH>(PO_LDS_CAP_MAX)));
            attr_set[dev] = true;
        }
        hipLaunchKernelGGL((pose_opt_kernel<TH, true>), dim3(n_problems), dim3(TH), lds, s, d_offsets, (const KeyPointPOD *)d_keys_un, d_u_right,
                           d_has_point, d_Xw, d_Tcw, d_outlier, d_n_inliers, (const float *)st->sig.p, p->fx, p->fy, p->cx, p->cy, p->bf, cap);
    } else {
        hipLaunchKernelGGL((pose_opt_kernel<TH, false>), dim3(n_problems), dim3(TH), pose_lds_bytes<TH>(0), s, d_offsets, (const KeyPointPOD *)d_keys_un,
                           d_u_right, d_has_point, d_Xw, d_Tcw, d_outlier, d_n_inliers, (const float *)st->sig.p, p->fx, p->fy, p->cx, p->cy, p->bf, 0);
    }
    ORBFE_HIP_TRY(ctx, hipGetLastError());
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

#ifdef ORBFE_POSE_TIMING
extern "C" int orbfe_pose_debug_cycles(long long *dst, int reset)
try {
    if (hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_pose_cycles), sizeof(long long) * 8) != hipSuccess) return -1;
    if (reset) { long long z[8] = {}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_pose_cycles), z, sizeof(z)) != hipSuccess) return -1; }
    return 0;
} ORBFE_CATCH(nullptr)
#endif

extern "C" int orbfe_pose_optimization_batch(orbfe_context *ctx, int n_problems, const int32_t *offsets, float *Tcw,
                                             const orbfe_keypoint *keys_un, const float *u_right, const uint8_t *has_point,
                                             const float *Xw, uint8_t *outlier, int32_t *n_inliers)
try {
    ORBFE_ENTRY(ctx);
    if (!ctx || n_problems < 0) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "bad argument");
    if (n_problems == 0) return ORBFE_OK;
    if (!offsets || !Tcw || !outlier || !n_inliers) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null argument");
    const int total = offsets[n_problems];
    const orbfe_params *p = &ctx->params;
    int max_n = 0;
    for (int k = 0; k < n_problems; k++) {
        if (offsets[k + 1] < offsets[k] || offsets[0] != 0) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "offsets must start at 0 and not decrease");
        max_n = std::max(max_n, offsets[k + 1] - offsets[k]);
    }
    if (total > 0 && (!keys_un || !u_right || !has_point || !Xw)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null argument");
    for (int i = 0; i < total; i++)
        if (has_point[i] && (keys_un[i].octave < 0 || keys_un[i].octave >= p->nlevels))
            return orbfe_fail(ctx, ORBFE_ERR_INVALID, "keypoint %d has octave %d outside the context's %d levels", i, keys_un[i].octave, p->nlevels);
    orbfe_pose_state *st = orbfe_ctx_pose_state(ctx);
    hipStream_t s;
    if (const int rc = orbfe_enqueue_on(ctx, nullptr, false, &s)) return rc;
    // the staging block: results first, then the inputs; its host image is the state's pinned block, kept between calls
    const size_t np = (size_t)n_problems, tn = (size_t)total;
    orbfe::StageLayout L;
    const auto f_T = L.result<float>(np, 16); const auto f_n = L.result<int32_t>(np); const auto f_out = L.result<uint8_t>(tn);
    const auto f_off = L.input<int32_t>(np + 1); const auto f_keys = L.input<orbfe_keypoint>(tn); const auto f_ur = L.input<float>(tn);
    const auto f_has = L.input<uint8_t>(tn); const auto f_xw = L.input<float>(tn, 3);
    const size_t bytes = L.bytes();
    if (st->blk.ensure(bytes)) return orbfe_fail(ctx, ORBFE_ERR_HIP, "pose scratch allocation failed");
    if (st->h_bytes < bytes) {
        if (st->h_blk) (void)hipHostFree(st->h_blk);
        st->h_blk = nullptr; st->h_bytes = 0;
        ORBFE_HIP_TRY(ctx, hipHostMalloc((void **)&st->h_blk, bytes, hipHostMallocDefault));
        st->h_bytes = bytes;
    }
    StageBlock blk(L, st->blk, st->h_blk);
    blk.put(f_T, Tcw, 16 * np); blk.put(f_off, offsets, np + 1); blk.put(f_out, outlier, tn); // entries without a point keep the caller's value
    blk.put(f_keys, keys_un, tn); blk.put(f_ur, u_right, tn); blk.put(f_has, has_point, tn); blk.put(f_xw, Xw, 3 * tn);
    ORBFE_HIP_TRY(ctx, blk.upload(s));
    int rc = orbfe_enqueue_pose_optimization(ctx, n_problems, blk.dev(f_off), blk.dev(f_keys), blk.dev(f_ur), blk.dev(f_has), blk.dev(f_xw), blk.dev(f_T),
                                             blk.dev(f_out), blk.dev(f_n), max_n, nullptr);
    if (rc != ORBFE_OK) return rc;
    ORBFE_HIP_TRY(ctx, blk.download(s));
    ORBFE_HIP_TRY(ctx, hipStreamSynchronize(s));
    // problems with fewer than 3 correspondences leave their pose untouched on the device (the reference returns
    // before SetPose, src/Optimizer.cc:404-405)
    blk.get(f_T, Tcw, 16 * np); blk.get(f_n, n_inliers, np); blk.get(f_out, outlier, tn);
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

extern "C" int orbfe_pose_optimization(orbfe_context *ctx, float *Tcw, int n, const orbfe_keypoint *keys_un, const float *u_right,
                                       const uint8_t *has_point, const float *Xw, uint8_t *outlier, int *n_inliers)
try {
    ORBFE_ENTRY(ctx);
    if (!n_inliers || n < 0) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "bad argument");
    const int32_t off[2] = {0, n};
    int32_t ninl = 0;
    const int rc = orbfe_pose_optimization_batch(ctx, 1, off, Tcw, keys_un, u_right, has_point, Xw, outlier, &ninl);
    *n_inliers = ninl;
    return rc;
} ORBFE_CATCH(ctx)
