// orbfe_lba.hip -- Optimizer::LocalBundleAdjustment (src/Optimizer.cc:566-822) of LocalMapping::Run on device-resident keyframes and
// the map-point table, asynchronous on the caller's stream.  The graph walk of :499-548 stays the caller's and arrives as roles and
// observation lists (the CSR of orbfe_enqueue_update_map_points).
//
// One launch of one workgroup of LBA_THREADS threads drives both optimize() calls, all 15 iterations and every Levenberg trial; no
// workgroup waits for another and the host does nothing in between.  FP64.  Every floating-point sum has an order fixed by the inputs:
//   per point     its owner thread walks the point's list in order: Hll, b_l, and per edge Hpl and the edge's share of Hpp / b_p (scratch)
//   per keyframe  a wave walks the free keyframe's edges in edge order (a counting sort by keyframe, built once per call): Hpp, b_p, and
//                 per trial its block row of the Schur complement, following each edge's point list to the partner blocks
//   totals        lba_block_sum: wave butterflies, then the waves in order
// The reduced system ((6K + 1) x 6K doubles, right-hand side as the last row) lives in the LDS for up to ORBFE_LBA_LDS_KEYFRAMES free
// keyframes and in the context's scratch above that; the host picks the variant from max_free_kfs.
//
// g2o call map:  lba_errors                          = computeActiveErrors + activeRobustChi2
//                lba_linearize                       = BlockSolver<6,3>::buildSystem (core/block_solver.hpp:502-570)
//                lba_solve                           = setLambda + BlockSolver::solve (:353-486), LinearSolverEigen as a dense LDLT without pivoting
//                lba_apply                           = SparseOptimizer::update (VertexSE3Expmap / VertexSBAPointXYZ::oplusImpl)
//                lba_optimize                        = SparseOptimizer::optimize + OptimizationAlgorithmLevenberg::solve
//                lba_classify                        = the two chi2 / isDepthPositive loops (:716-746, :759-787)
// A trial evaluates errors only; an accepted trial is linearised in a pass of its own (a rejected one then costs no Jacobian, and the
// 48 doubles per edge of the linearisation need no second buffer).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "orbfe_device.h"
#include "orbfe_host.h"

#include "orbfe_lba_blocks.hpp"

#pragma clang fp contract(fast)


extern "C" int orbfe_enqueue_local_bundle_adjustment(orbfe_context *ctx, const orbfe_ba_keyframe *d_kfs, const uint8_t *d_role, int n_kfs, int max_free_kfs,
                                                     float *d_Tcw, int n_pts, const int32_t *d_row, int n_rows, const int32_t *d_obs_off,
                                                     const int32_t *d_obs_kf, const int32_t *d_obs_idx, int n_obs, float *d_pos,
                                                     orbfe_obs_keyframe *d_obs_kfs, uint8_t *d_edge_code, double *d_edge_chi2, int32_t *d_erase,
                                                     int32_t *d_n_erase, orbfe_lba_info *d_info, int32_t *d_status, void *stream)
try {
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    ORBFE_ENTRY(ctx);
    if (!d_info || !d_status || !d_n_erase) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null argument");
    if (n_kfs < 0 || n_pts < 0 || n_rows < 0 || n_obs < 0 || max_free_kfs < 0) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "negative count");
    if (max_free_kfs > n_kfs) max_free_kfs = n_kfs;
    if (!d_row && n_rows < n_pts) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "n_rows = %d < n_pts = %d without d_row", n_rows, n_pts);
    if (n_kfs > 0 && (!d_kfs || !d_role || !d_Tcw)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null keyframe array");
    if (n_pts > 0 && (!d_obs_off || !d_pos)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null point array");
    if (n_obs > 0 && (!d_obs_kf || !d_obs_idx || !d_edge_code || !d_erase)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null observation array");
    const orbfe_params *cp = &ctx->params;
    if (cp->nlevels < 1 || cp->nlevels > ORBFE_MAX_LEVELS) return orbfe_fail(ctx, ORBFE_ERR_UNSUPPORTED, "nlevels = %d", cp->nlevels);
    hipStream_t s;
    if (const int rc = orbfe_enqueue_on(ctx, stream, false, &s)) return rc;
    LbaArgs a = {};
    a.kfs = d_kfs; a.role = d_role; a.Tcw = d_Tcw; a.row = d_row; a.obs_off = d_obs_off; a.obs_kf = d_obs_kf; a.obs_idx = d_obs_idx;
    a.pos = d_pos; a.obs_kfs = d_obs_kfs; a.edge_code = d_edge_code; a.edge_chi2 = d_edge_chi2; a.erase = d_erase; a.n_erase = d_n_erase;
    a.status = d_status; a.info = d_info;
    a.n_kfs = n_kfs; a.max_free = max_free_kfs; a.n_pts = n_pts; a.n_rows = n_rows; a.n_obs = n_pts > 0 ? n_obs : 0; a.nlevels = cp->nlevels;
    for (int l = 0; l < ORBFE_MAX_LEVELS; l++) a.inv_sigma2[l] = l < cp->nlevels ? ctx->plan.inv_sigma2[l] : 0.f;
    a.fx = cp->fx; a.fy = cp->fy; a.cx = cp->cx; a.cy = cp->cy; a.bf = cp->bf;
    a.delta_mono = (double)(float)std::sqrt(5.991);   // const float thHuberMono = sqrt(5.991) (:613-614)
    a.delta_stereo = (double)(float)std::sqrt(7.815);
    // the scratch, carved from one grow-only buffer
    const bool in_lds = max_free_kfs <= ORBFE_LBA_LDS_KEYFRAMES;
    const size_t bytes = lba_carve(a, nullptr, !in_lds);
    if (ctx->lba_scratch.ensure(bytes)) return orbfe_fail(ctx, ORBFE_ERR_HIP, "bundle adjustment scratch allocation of %zu bytes failed", bytes);
    lba_carve(a, (uint8_t *)ctx->lba_scratch.p, !in_lds);
    if (in_lds) {
        // per device, and set on every call: remembering it would be state shared between the host threads of different contexts
        ORBFE_HIP_TRY(ctx, hipFuncSetAttribute((const void *)lba_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LBA_LDS_REQUEST));
        hipLaunchKernelGGL((lba_kernel<true>), dim3(1), dim3(LBA_THREADS), std::max<size_t>(lba_system_bytes(max_free_kfs), 8), s, a);
    } else {
        hipLaunchKernelGGL((lba_kernel<false>), dim3(1), dim3(LBA_THREADS), 8, s, a);
    }
    ORBFE_HIP_TRY(ctx, hipGetLastError());
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

#ifdef ORBFE_LBA_TIMING
extern "C" int orbfe_lba_debug_cycles(long long *dst, int reset)
try {
    if (hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_lba_cycles), sizeof(long long) * 8) != hipSuccess) return -1;
    if (reset) { long long z[8] = {}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_lba_cycles), z, sizeof(z)) != hipSuccess) return -1; }
    return 0;
} ORBFE_CATCH(nullptr)
#endif

extern "C" int orbfe_local_bundle_adjustment(orbfe_context *ctx, const orbfe_keypoint *const *keys_un, const float *const *u_right, const int32_t *kf_n,
                                             const uint8_t *role, int n_kfs, float *Tcw, int n_pts, const int32_t *row, int n_rows,
                                             const int32_t *obs_off, const int32_t *obs_kf, const int32_t *obs_idx, int n_obs, float *pos,
                                             float *Ow, uint8_t *edge_code, double *edge_chi2, int32_t *erase, int32_t *n_erase, orbfe_lba_info *info)
try {
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    ORBFE_ENTRY(ctx);
    if (!info || !n_erase) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null argument");
    if (n_kfs < 0 || n_pts < 0 || n_rows < 0 || n_obs < 0) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "negative count");
    if (!row && n_rows < n_pts) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "n_rows = %d < n_pts = %d without row", n_rows, n_pts);
    if (n_kfs > 0 && (!keys_un || !u_right || !kf_n || !role || !Tcw)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null keyframe array");
    if (n_pts > 0 && (!obs_off || !pos)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null point array");
    if (n_obs > 0 && (!obs_kf || !obs_idx || !edge_code || !erase)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null observation array");
    int max_free = 0;
    size_t n_keys = 0;
    for (int k = 0; k < n_kfs; k++) {
        if (kf_n[k] < 0 || (kf_n[k] > 0 && (!keys_un[k] || !u_right[k]))) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "keyframe %d: negative n or null array", k);
        max_free += role[k] == ORBFE_BA_LOCAL;
        n_keys += (size_t)kf_n[k];
    }
    hipStream_t s;
    if (const int rc = orbfe_enqueue_on(ctx, nullptr, false, &s)) return rc;
    // the staging block: results first, then the inputs
    orbfe::StageLayout L;
    const auto f_info = L.result<orbfe_lba_info>(1); const auto f_cnt = L.result<int32_t>(2); // n_erase, status
    const auto f_T = L.result<float>(n_kfs, 16); const auto f_pos = L.result<float>(n_rows, 3); const auto f_okf = L.result<orbfe_obs_keyframe>(n_kfs);
    const auto f_code = L.result<uint8_t>(n_obs); const auto f_chi = L.result<double>(n_obs); const auto f_erase = L.result<int32_t>(n_obs, 2);
    const auto f_rec = L.input<orbfe_ba_keyframe>(n_kfs); const auto f_role = L.input<uint8_t>(n_kfs); const auto f_row = L.input<int32_t>(n_pts);
    const auto f_off = L.input<int32_t>((size_t)n_pts + 1); const auto f_kf = L.input<int32_t>(n_obs); const auto f_idx = L.input<int32_t>(n_obs);
    const auto f_keys = L.input<orbfe_keypoint>(n_keys); const auto f_ur = L.input<float>(n_keys);
    if (ctx->sync_stage.ensure(L.bytes())) return orbfe_fail(ctx, ORBFE_ERR_HIP, "bundle adjustment staging allocation failed");
    StageBlock blk(L, ctx->sync_stage);
    if (n_kfs > 0) {
        blk.put(f_T, Tcw, 16 * (size_t)n_kfs);
        blk.put(f_role, role, n_kfs);
        orbfe_ba_keyframe *rec = blk.host(f_rec);
        size_t at = 0;
        for (int k = 0; k < n_kfs; k++) {
            rec[k].keys_un = blk.dev(f_keys) + at;
            rec[k].u_right = blk.dev(f_ur) + at;
            rec[k].n = kf_n[k];
            blk.put(f_keys, keys_un[k], kf_n[k], at);
            blk.put(f_ur, u_right[k], kf_n[k], at);
            at += (size_t)kf_n[k];
        }
    }
    if (pos) blk.put(f_pos, pos, 3 * (size_t)n_rows);
    if (n_pts > 0) {
        if (row) blk.put(f_row, row, n_pts);
        blk.put(f_off, obs_off, (size_t)n_pts + 1);
    }
    blk.put(f_kf, obs_kf, n_obs); blk.put(f_idx, obs_idx, n_obs);
    ORBFE_HIP_TRY(ctx, blk.upload(s));
    const int rc = orbfe_enqueue_local_bundle_adjustment(ctx, blk.dev(f_rec), blk.dev(f_role), n_kfs, max_free, blk.dev(f_T), n_pts, row ? blk.dev(f_row) : nullptr, n_rows,
                                                         blk.dev(f_off), blk.dev(f_kf), blk.dev(f_idx), n_obs, blk.dev(f_pos), Ow ? blk.dev(f_okf) : nullptr,
                                                         blk.dev(f_code), edge_chi2 ? blk.dev(f_chi) : nullptr, blk.dev(f_erase), blk.dev(f_cnt), blk.dev(f_info),
                                                         blk.dev(f_cnt) + 1, nullptr);
    if (rc != ORBFE_OK) return rc;
    ORBFE_HIP_TRY(ctx, blk.download(s));
    ORBFE_HIP_TRY(ctx, hipStreamSynchronize(s));
    int32_t cnt[2];
    blk.get(f_cnt, cnt, 2); blk.get(f_info, info, 1);
    *n_erase = cnt[0];
    blk.get(f_T, Tcw, 16 * (size_t)n_kfs);
    if (pos) blk.get(f_pos, pos, 3 * (size_t)n_rows);
    if (Ow && info->n_mono + info->n_stereo > 0 && cnt[1] != ORBFE_ERR_CAPACITY) { // a call without an edge rewrites no keyframe
        const orbfe_obs_keyframe *okf = blk.host(f_okf);
        for (int k = 0; k < n_kfs; k++)
            if (role[k] == ORBFE_BA_LOCAL || role[k] == ORBFE_BA_LOCAL_HELD) memcpy(Ow + 3 * (size_t)k, okf[k].Ow, sizeof(float) * 3);
    }
    blk.get(f_code, edge_code, n_obs);
    if (edge_chi2) blk.get(f_chi, edge_chi2, n_obs);
    blk.get(f_erase, erase, 2 * (size_t)n_obs);
    if (cnt[1] == ORBFE_ERR_CAPACITY) return orbfe_fail(ctx, cnt[1], "more free keyframes than the bound");
    if (cnt[1] != 0) return orbfe_fail(ctx, cnt[1], "a faulty observation, point or role (see the edge codes)");
    return ORBFE_OK;
} ORBFE_CATCH(ctx)
