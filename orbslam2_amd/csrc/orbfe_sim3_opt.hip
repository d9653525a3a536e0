// orbfe_sim3_opt.hip -- Optimizer::OptimizeSim3 (src/Optimizer.cc:1090-1285) of LoopClosing::ComputeSim3 (src/LoopClosing.cc:362) on two
// device-resident keyframes, asynchronous on the caller's stream: SearchBySim3's d_match12 goes in as it lies in HBM, what comes back is
// a count, eight doubles and d_match12 with the outliers cleared.
//
// One workgroup of 256 threads per call, the shape of pose_opt_kernel (orbfe_pose.hip): one free vertex (the Sim3, 7 dof), the points
// fixed, g2o's Levenberg with a dense 7 x 7 LDLT, Huber, chi-square classification, FP64.  Per correspondence two binary edges whose
// Jacobians are g2o's NUMERIC ones (linearizeOplus of both edge classes is commented out in the reference): 2 x 15 error evaluations per
// correspondence and pass, so the correspondences are compacted first, in ascending keypoint slot, into a dense table -- in LDS when
// KF1 has at most ORBFE_SIM3_OPT_LDS_SLOTS slots, else in the context's scratch in HBM (the host selects the variant from kf1->n, the
// count is known only to the kernel).  Every lane repeats the per-trial serial part (LDLT, exponential, acceptance); one evaluation pass
// yields the robust chi2 and the normal equations at the trial estimate, which an accepted trial hands to the next iteration.  All block
// sums have a fixed order: the result is bit-reproducible run to run.
//
// g2o call map:  sim3_eval_pass (orbfe_sim3_blocks.hpp) = computeActiveErrors + activeRobustChi2 + buildSystem
//                solve_ldlt<7> (orbfe_pose_blocks.hpp)  = LinearSolverDense::solve (Eigen::LDLT)
//                sim3_oplus                             = SparseOptimizer::update -> VertexSim3Expmap::oplusImpl
//                the do/while                           = OptimizationAlgorithmLevenberg::solve (core/optimization_algorithm_levenberg.cpp:61-164)
//                sim3_optimize's for                    = SparseOptimizer::optimize (core/sparse_optimizer.cpp:354-419)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "orbfe_device.h"
#include "orbfe_host.h"
#include "orbfe_cvmat.hpp"

#include "orbfe_sim3_blocks.hpp" // Sim3D ... sim3_eval_pass, and this stage's fp contract(fast) pragma

#pragma clang fp contract(fast)

namespace {

constexpr int SO_THREADS = 256;

struct Sim3OptArgs {
    const KeyPointPOD *keys1, *keys2;
    const float *pos1, *pos2;
    const int32_t *valid1, *valid2;
    const int32_t *prior12;
    int32_t *match12;
    double *S12;
    int32_t *n_inliers, *status;
    void *table; // the HBM variant's correspondence table (the context's scratch)
    float T1w[12], T2w[12], R12[9], t12[3], s12, th2;
    double delta; // (double)(float)sqrt(th2)
    float inv_sigma2[ORBFE_MAX_LEVELS];
    float fx, fy, cx, cy;
    int32_t n1, n2, nlevels, cap, fix_scale;
    int32_t iterations, more_iterations_outliers, more_iterations_clean, min_inliers;
};

// dynamic LDS: the row partials, the two systems (accepted / trial), the pass's Sim3 list, then the table
__host__ __device__ constexpr size_t sim3_lds_bytes(int cap)
{
    return sizeof(double) * ((SO_THREADS / 16) * S3_NVAL + 2 * S3_NVAL + S3_NSIM * S3_SIM_STRIDE) + corr_table_bytes(cap);
}
static_assert(sim3_lds_bytes(ORBFE_SIM3_OPT_LDS_SLOTS) <= pose_lds_bytes<256>(PO_LDS_CAP_MAX), "no more LDS than pose_opt_kernel's largest launch requests");

struct Sim3Run { // what the solver carries between the two optimize() calls
    Sim3D est, last_eval;
    int cur;
};

// SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg over the table's active correspondences
template <int THREADS>
__device__ void sim3_optimize(const CorrTable &T, Sim3Run &r, int iterations, bool fix_scale, const CamK &cam, double delta, double *s_sims, double *s_rows,
                              double *s_tot)
{
    double chi_s, cnt_s;
    Sim3D est = r.est, last_eval = r.est;
    int cur = r.cur;
    sim3_eval_pass<THREADS>(T, est, fix_scale, cam, delta, s_sims, s_rows, s_tot + cur * S3_NVAL, chi_s, cnt_s);
    if (cnt_s > 0.0) { // otherwise optimize() returns before doing anything (no active vertex)
        double current_chi = chi_s;
        double lambda = -1.0, ni = 2.0;
        int lm_bad = 0;
        double x[7] = {0, 0, 0, 0, 0, 0, 0};
        for (int it = 0; it < iterations; it++) {
            last_eval = est; // computeActiveErrors at the current estimate
            const double ini_chi = current_chi;
            const double *Hb = s_tot + cur * S3_NVAL;
            if (it == 0) {
                const double dg[7] = {Hb[0], Hb[7], Hb[13], Hb[18], Hb[22], Hb[25], Hb[27]};
                double mx = 0.0;
#pragma unroll
                for (int j = 0; j < 7; j++) mx = fmax(fabs(dg[j]), mx);
                lambda = 1e-5 * mx;
                ni = 2.0;
                lm_bad = 0;
            }
            double rho = 0.0;
            int qmax = 0;
            do {
                const bool ok2 = solve_ldlt<7>(Hb, lambda, x);
                double scale = 0.0; // computeScale(), with the b of the system that produced x
#pragma unroll
                for (int j = 0; j < 7; j++) scale += x[j] * (lambda * x[j] + Hb[28 + j]);
                scale += 1e-3;
                const Sim3D trial = sim3_oplus(x, fix_scale, est);
                sim3_eval_pass<THREADS>(T, trial, fix_scale, cam, delta, s_sims, s_rows, s_tot + (cur ^ 1) * S3_NVAL, chi_s, cnt_s);
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
                    Hb = s_tot + cur * S3_NVAL;
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
    r.est = est; r.last_eval = last_eval; r.cur = cur;
}

// e12->chi2() > th2 || e21->chi2() > th2 over the active correspondences, at the last evaluated estimate (g2o pops the vertex after a
// rejected trial and does not recompute the errors).  A bad one loses its d_match12 entry; with `remove` its edges leave the graph.
// Returns the number of bad ones in every lane; *n_active_out the number of active ones before the call.
template <int THREADS>
__device__ int sim3_classify(const CorrTable &T, const Sim3D &at, const CamK &cam, double th2, bool remove, int32_t *match12, int *s_cnt, int *n_active_out)
{
    const Sim3D inv = sim3_inverse(at);
    int bad = 0, active = 0;
    for (int k = threadIdx.x; k < T.n; k += THREADS) {
        if (corr_state(T, k) != 1) continue;
        double P1[3], P2[3], obs1[2], obs2[2], info1, info2, e12[2], e21[2];
        corr_load(T, k, P1, P2, obs1, obs2, info1, info2);
        sim3_edge_error(at, cam, P2, obs1, e12);
        sim3_edge_error(inv, cam, P1, obs2, e21);
        const double chi12 = e12[0] * (info1 * e12[0]) + e12[1] * (info1 * e12[1]);
        const double chi21 = e21[0] * (info2 * e21[0]) + e21[1] * (info2 * e21[1]);
        active++;
        if (chi12 > th2 || chi21 > th2) {
            match12[corr_slot(T, k)] = -1;
            if (remove) corr_remove(T, k);
            bad++;
        }
    }
    if (threadIdx.x == 0) { s_cnt[0] = 0; s_cnt[1] = 0; }
    __syncthreads();
    for (int off = 32; off >= 1; off >>= 1) { bad += __shfl_xor(bad, off, 64); active += __shfl_xor(active, off, 64); }
    if ((threadIdx.x & 63) == 0) { // integer counts: the order of the waves does not matter
        if (bad) atomicAdd(&s_cnt[0], bad);
        if (active) atomicAdd(&s_cnt[1], active);
    }
    __syncthreads();
    bad = s_cnt[0];
    *n_active_out = s_cnt[1];
    __syncthreads(); // s_cnt is cleared again by the next call
    return bad;
}

template <int THREADS, bool IN_LDS>
__global__ __launch_bounds__(THREADS) void sim3_opt_kernel(const Sim3OptArgs a)
{
    extern __shared__ double s_dyn[];
    double *s_rows = s_dyn;                             // [THREADS/16][40]
    double *s_tot = s_rows + (THREADS / 16) * S3_NVAL;  // [2][40]
    double *s_sims = s_tot + 2 * S3_NVAL;               // [15][16]
    __shared__ int s_wave[THREADS / 64];
    __shared__ int s_cnt[2];
    __shared__ int s_invalid;
    CorrTable T;
    T.cap = a.cap;
    if constexpr (IN_LDS) T.f = (float *)(s_sims + S3_NSIM * S3_SIM_STRIDE);
    else T.f = (float *)a.table;
    T.tag = (uint32_t *)(T.f + 12 * (size_t)a.cap);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_invalid = 0;
    __syncthreads();

    // the input Sim3: g2o::Sim3(Converter::toMatrix3d(R12), Converter::toVector3d(t12), s12) (src/LoopClosing.cc:341)
    Sim3Run run;
    {
        double R[3][3], t[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int j = 0; j < 3; j++) R[i][j] = (double)a.R12[3 * i + j];
            t[i] = (double)a.t12[i];
        }
        run.est = sim3_from_rts(R, t, (double)a.s12);
        run.last_eval = run.est;
        run.cur = 0;
    }
    const Sim3D input = run.est;
    const CamK cam = {(double)a.fx, (double)a.fy, (double)a.cx, (double)a.cy};
    const double th2 = (double)a.th2;
    const bool fix_scale = a.fix_scale != 0;

    // the correspondences, in ascending slot (:1143-1222); d_match12 becomes the merge of d_prior12 and what it held
    float T1w[12], T2w[12];
#pragma unroll
    for (int k = 0; k < 12; k++) { T1w[k] = a.T1w[k]; T2w[k] = a.T2w[k]; }
    int n_corr = 0;
    for (int c0 = 0; c0 < a.n1; c0 += THREADS) {
        const int i = c0 + threadIdx.x;
        bool edge = false;
        int m = -1, o1 = 0, o2 = 0;
        if (i < a.n1) {
            const int pr = a.prior12 ? a.prior12[i] : -1;
            m = pr >= 0 ? pr : a.match12[i];
            if (m != -1) {
                bool ok = m >= 0 && m < a.n2; // checked before it becomes an address
                if (ok) {
                    o1 = a.keys1[i].octave; o2 = a.keys2[m].octave;
                    ok = o1 >= 0 && o1 < a.nlevels && o2 >= 0 && o2 < a.nlevels;
                }
                if (!ok) { s_invalid = 1; m = -1; } // every lane that writes writes this value
                else edge = a.valid1[i] != 0 && a.valid2[m] != 0; // the reference's `continue` keeps vpMatches1[i]
            }
            a.match12[i] = m;
        }
        const unsigned long long vote = __ballot(edge);
        if (lane == 0) s_wave[wave] = __popcll(vote);
        __syncthreads();
        int before = n_corr, total = 0;
#pragma unroll
        for (int w = 0; w < THREADS / 64; w++) {
            const int cw = s_wave[w];
            if (w < wave) before += cw;
            total += cw;
        }
        if (edge) {
            const int k = before + __popcll(vote & ((1ull << lane) - 1)); // < number of edges so far <= i < cap
            const float X1[3] = {a.pos1[3 * (size_t)i], a.pos1[3 * (size_t)i + 1], a.pos1[3 * (size_t)i + 2]};
            const float X2[3] = {a.pos2[3 * (size_t)m], a.pos2[3 * (size_t)m + 1], a.pos2[3 * (size_t)m + 2]};
            const KeyPointPOD k1 = a.keys1[i], k2 = a.keys2[m];
            // P3D1c = R1w * P3D1w + t1w: a float cv::Mat product with its `+ C` form (:1162, :1170)
            const float v[12] = {row_dot_plus<0>(T1w, X1), row_dot_plus<1>(T1w, X1), row_dot_plus<2>(T1w, X1),
                                 row_dot_plus<0>(T2w, X2), row_dot_plus<1>(T2w, X2), row_dot_plus<2>(T2w, X2),
                                 k1.x, k1.y, k2.x, k2.y, a.inv_sigma2[o1], a.inv_sigma2[o2]};
            corr_store(T, k, v, i);
        }
        n_corr += total;
        __syncthreads(); // s_wave is rewritten by the next chunk; after the last one: the table is complete
    }
    T.n = n_corr;

    int n_in = 0;
    bool failed = true;
    if (n_corr > 0) { // without an edge the vertex is not active: optimize() returns at once and nothing is classified
        sim3_optimize<THREADS>(T, run, a.iterations, fix_scale, cam, a.delta, s_sims, s_rows, s_tot);
        int n_active;
        const int n_bad = sim3_classify<THREADS>(T, run.last_eval, cam, th2, true, a.match12, s_cnt, &n_active);
        if (n_corr - n_bad >= a.min_inliers) { // :1255-1256
            failed = false;
            sim3_optimize<THREADS>(T, run, n_bad > 0 ? a.more_iterations_outliers : a.more_iterations_clean, fix_scale, cam, a.delta, s_sims, s_rows, s_tot);
            const int n_bad2 = sim3_classify<THREADS>(T, run.last_eval, cam, th2, false, a.match12, s_cnt, &n_active);
            n_in = n_active - n_bad2;
        }
    }
    if (threadIdx.x == 0) {
        sim3_store(failed ? input : run.est, a.S12); // the reference leaves g2oS12 untouched when it returns 0 early
        *a.n_inliers = failed ? 0 : n_in;
        *a.status = s_invalid ? ORBFE_ERR_INVALID : 0;
    }
}

} // namespace

extern "C" int orbfe_enqueue_optimize_sim3(orbfe_context *ctx, const orbfe_grid_keyframe *kf1, const float *T1w, const float *d_pos1,
                                           const int32_t *d_valid1, const orbfe_grid_keyframe *kf2, const float *T2w, const float *d_pos2,
                                           const int32_t *d_valid2, float s12, const float *R12, const float *t12, float th2, int fix_scale,
                                           const orbfe_sim3_opt_params *params, const int32_t *d_prior12, int32_t *d_match12, double *d_S12,
                                           int32_t *d_n_inliers, int32_t *d_status, void *stream)
try {
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    ORBFE_ENTRY(ctx);
    if (!kf1 || !kf2 || !T1w || !T2w || !R12 || !t12 || !d_S12 || !d_n_inliers || !d_status) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null argument");
    const int n1 = kf1->n, n2 = kf2->n;
    if (n1 < 0 || n1 > 65535 || n2 < 0 || n2 > 65535) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "keyframe with %d / %d keypoints (0 .. 65535)", n1, n2);
    if (n1 > 0 && (!kf1->keys_un || !d_pos1 || !d_valid1 || !d_match12)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null array of keyframe 1");
    if (n2 > 0 && (!kf2->keys_un || !d_pos2 || !d_valid2)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null array of keyframe 2");
    if (!(th2 > 0)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "th2 must be positive");
    const orbfe_sim3_opt_params defaults = {5, 10, 5, 10}; // src/Optimizer.cc:60-70
    const orbfe_sim3_opt_params P = params ? *params : defaults;
    if (P.iterations < 1 || P.more_iterations_outliers < 1 || P.more_iterations_clean < 1 || P.min_inliers < 1)
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "every field of orbfe_sim3_opt_params must be at least 1");
    const orbfe_params *cp = &ctx->params;
    if (cp->nlevels < 1 || cp->nlevels > ORBFE_MAX_LEVELS) return orbfe_fail(ctx, ORBFE_ERR_UNSUPPORTED, "nlevels = %d", cp->nlevels);
    hipStream_t s;
    if (const int rc = orbfe_enqueue_on(ctx, stream, false, &s)) return rc;
    Sim3OptArgs a;
    a.keys1 = (const KeyPointPOD *)kf1->keys_un; a.keys2 = (const KeyPointPOD *)kf2->keys_un;
    a.pos1 = d_pos1; a.pos2 = d_pos2; a.valid1 = d_valid1; a.valid2 = d_valid2;
    a.prior12 = d_prior12; a.match12 = d_match12; a.S12 = d_S12; a.n_inliers = d_n_inliers; a.status = d_status;
    a.table = nullptr;
    for (int k = 0; k < 12; k++) { a.T1w[k] = T1w[k]; a.T2w[k] = T2w[k]; }
    for (int k = 0; k < 9; k++) a.R12[k] = R12[k];
    for (int k = 0; k < 3; k++) a.t12[k] = t12[k];
    a.s12 = s12; a.th2 = th2;
    a.delta = (double)(float)std::sqrt((double)th2); // const float deltaHuber = sqrt(th2) (:1139)
    for (int l = 0; l < ORBFE_MAX_LEVELS; l++) a.inv_sigma2[l] = l < cp->nlevels ? ctx->plan.inv_sigma2[l] : 0.f;
    a.fx = cp->fx; a.fy = cp->fy; a.cx = cp->cx; a.cy = cp->cy;
    a.n1 = n1; a.n2 = n2; a.nlevels = cp->nlevels; a.fix_scale = fix_scale != 0;
    a.cap = (std::max(n1, 1) + 3) & ~3;
    a.iterations = P.iterations; a.more_iterations_outliers = P.more_iterations_outliers; a.more_iterations_clean = P.more_iterations_clean;
    a.min_inliers = P.min_inliers;
    constexpr int TH = SO_THREADS;
    if (n1 <= ORBFE_SIM3_OPT_LDS_SLOTS) {
        static bool attr_set[64] = {}; // the attribute is per device
        const int dev = cp->device;
        if (dev >= 0 && dev < 64 && !attr_set[dev]) {
            ORBFE_HIP_TRY(ctx, hipFuncSetAttribute((const void *)sim3_opt_kernel<TH, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                   (int)sim3_lds_bytes(ORBFE_SIM3_OPT_LDS_SLOTS)));
            attr_set[dev] = true;
        }
        hipLaunchKernelGGL((sim3_opt_kernel<TH, true>), dim3(1), dim3(TH), sim3_lds_bytes(a.cap), s, a);
    } else {
        if (ctx->sim3_opt_scratch.ensure(corr_table_bytes(a.cap))) return orbfe_fail(ctx, ORBFE_ERR_HIP, "Sim3 optimisation scratch allocation failed");
        a.table = ctx->sim3_opt_scratch.p;
        hipLaunchKernelGGL((sim3_opt_kernel<TH, false>), dim3(1), dim3(TH), sim3_lds_bytes(0), s, a);
    }
    ORBFE_HIP_TRY(ctx, hipGetLastError());
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

extern "C" int orbfe_optimize_sim3(orbfe_context *ctx, const orbfe_keypoint *keys_un1, int n1, const float *T1w, const float *pos1,
                                   const int32_t *valid1, const orbfe_keypoint *keys_un2, int n2, const float *T2w, const float *pos2,
                                   const int32_t *valid2, float s12, const float *R12, const float *t12, float th2, int fix_scale,
                                   const orbfe_sim3_opt_params *params, const int32_t *prior12, int32_t *match12, double *S12, int *n_inliers)
try {
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    ORBFE_ENTRY(ctx);
    if (!T1w || !T2w || !R12 || !t12 || !S12 || !n_inliers) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null argument");
    if (n1 < 0 || n1 > 65535 || n2 < 0 || n2 > 65535) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "keyframe with %d / %d keypoints (0 .. 65535)", n1, n2);
    if (n1 > 0 && (!keys_un1 || !pos1 || !valid1 || !match12)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null array of keyframe 1");
    if (n2 > 0 && (!keys_un2 || !pos2 || !valid2)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null array of keyframe 2");
    if (!(th2 > 0)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "th2 must be positive");
    if (params && (params->iterations < 1 || params->more_iterations_outliers < 1 || params->more_iterations_clean < 1 || params->min_inliers < 1))
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "every field of orbfe_sim3_opt_params must be at least 1");
    hipStream_t s;
    if (const int rc = orbfe_enqueue_on(ctx, nullptr, false, &s)) return rc;
    // the staging block: results first, then the inputs
    orbfe::StageLayout L;
    const auto f_S = L.result<double>(8); const auto f_cnt = L.result<int32_t>(2); // n_inliers, status
    const auto f_match = L.result<int32_t>(n1);
    const auto f_prior = L.input<int32_t>(n1); const auto f_k1 = L.input<orbfe_keypoint>(n1);
    const auto f_k2 = L.input<orbfe_keypoint>(n2); const auto f_p1 = L.input<float>(n1, 3); const auto f_p2 = L.input<float>(n2, 3);
    const auto f_v1 = L.input<int32_t>(n1); const auto f_v2 = L.input<int32_t>(n2);
    if (ctx->sync_stage.ensure(L.bytes())) return orbfe_fail(ctx, ORBFE_ERR_HIP, "Sim3 optimisation staging allocation failed");
    StageBlock blk(L, ctx->sync_stage);
    blk.put(f_match, match12, n1);
    if (prior12) blk.put(f_prior, prior12, n1);
    blk.put(f_k1, keys_un1, n1); blk.put(f_p1, pos1, 3 * (size_t)n1); blk.put(f_v1, valid1, n1);
    blk.put(f_k2, keys_un2, n2); blk.put(f_p2, pos2, 3 * (size_t)n2); blk.put(f_v2, valid2, n2);
    ORBFE_HIP_TRY(ctx, blk.upload(s));
    orbfe_grid_keyframe kf1 = {}, kf2 = {}; // only keys_un and n are read
    kf1.keys_un = blk.dev(f_k1); kf1.n = n1;
    kf2.keys_un = blk.dev(f_k2); kf2.n = n2;
    const int rc = orbfe_enqueue_optimize_sim3(ctx, &kf1, T1w, blk.dev(f_p1), blk.dev(f_v1), &kf2, T2w, blk.dev(f_p2), blk.dev(f_v2), s12, R12, t12, th2, fix_scale,
                                               params, prior12 ? blk.dev(f_prior) : nullptr, blk.dev(f_match), blk.dev(f_S), blk.dev(f_cnt), blk.dev(f_cnt) + 1,
                                               nullptr);
    if (rc != ORBFE_OK) return rc;
    ORBFE_HIP_TRY(ctx, blk.download(s));
    ORBFE_HIP_TRY(ctx, hipStreamSynchronize(s));
    blk.get(f_S, S12, 8);
    int32_t cnt[2];
    blk.get(f_cnt, cnt, 2);
    *n_inliers = cnt[0];
    blk.get(f_match, match12, n1);
    if (cnt[1] != 0) return orbfe_fail(ctx, cnt[1], "a match12 / prior12 entry outside [-1, n2) or a keypoint octave outside the context's %d levels", ctx->params.nlevels);
    return ORBFE_OK;
} ORBFE_CATCH(ctx)
