// orbfe_pnp_ransac.hip -- PnPsolver (src/PnPsolver.cc) of Tracking::Relocalization (src/Tracking.cc:1440-1600) for every candidate keyframe
// in one asynchronous call.  A hypothesis of PnPsolver::iterate depends on its four draws only, and Refine() on the inlier set of the
// record holder best(k) only, so all hypotheses of all candidates are evaluated at once, the record holders' refinements in a second
// pass, and iterate becomes a host walk over the fetched events (orbslam2_amd/host/PnPsolver.h).
//
// Five launches whatever n_cands is; launch boundaries are the only hand-off between workgroups:
//   pnp_filter_kernel   one workgroup per candidate: the constructor's filter (:68-111), survivors compacted in keypoint order into d_corr
//                       and into the correspondence table (6 floats per row, SoA, in the context's scratch), N and the iteration count
//   pnp_hyp_kernel      grid (chunks of PR_HPW = 64 hypotheses, candidates), one wave each: lane h runs EPnP of hypothesis h of the chunk
//                       (draws, compute_pose :478-526) on its own, then the wave walks the correspondences 64 at a time for each
//                       hypothesis of the chunk (CheckInliers :309-340); one 64-bit ballot per step is two words of the bit row and, by
//                       popcount, the count.  The table is staged in the LDS up to ORBFE_PNP_RANSAC_LDS_SLOTS and read from HBM above.
//                       The wave also writes zeros into its iterations' refinement rows.
//   pnp_scan_kernel     one wave per candidate: best_k, the prefix record holder of every iteration (:210-216), and the record holders
//                       compacted into a list in the context's scratch
//   pnp_refine_kernel   PR_REFINE_WAVES waves per candidate over that list (a handful of entries), so only record holders cost a wave
//                       with EPnP's private memory.  Refine() (:261-306): one lane runs EPnP over the hypothesis' inlier row, every
//                       n-row sum sequential in index order, then the wave's CheckInliers as above
//   pnp_events_kernel   one wave per candidate: the iterations at which iterate returns a refined pose, and the exhausted exit
// EPnP, CheckInliers and the draws are the ORBFE_CV_HD functions of orbslam2_amd/host/PnPsolver.h and CvMat.h, compiled here for the
// device: one definition for the kernels and the host form.  One lane per EPnP keeps its loops rolled and its branches the lane's own;
// the 12 x 12 Jacobi lives in the lane's private memory.  No atomics, plain vector stores, fixed orders everywhere: bit-reproducible run
// to run.  The arithmetic is DESIGN.md section 4p; this file is compiled without FMA contraction (the Makefile's -ffp-contract=off).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "orbfe_device.h"
#include "orbfe_host.h"
#include "orbfe_cvmat.hpp"
#include "../host/PnPsolver.h"

static_assert(sizeof(orbfe_pnp_candidate) == 64 && sizeof(orbfe_pnp_hypothesis) == 64 && sizeof(orbfe_pnp_refined) == 64, "record sizes are part of the ABI");

namespace {

using ORB_SLAM2::PnPCamera;
using ORB_SLAM2::PnPSet;
using ORB_SLAM2::PnPTable;
using ORB_SLAM2::PnPWork;

constexpr int PR_THREADS = 256; // filter and select
constexpr int PR_HPW = 64;      // hypotheses per wave of pnp_hyp_kernel: every lane runs one EPnP
constexpr int PR_REFINE_WAVES = 4; // waves per candidate of pnp_refine_kernel; a wave takes every 4th record holder (records are a handful)
constexpr int PR_FIELDS = 6;    // X Y Z u v max_error

struct PnpArgs {
    const KeyPointPOD *keys;
    const int32_t *n_keys;
    const orbfe_pnp_candidate *cands;
    const int32_t *its_for_n;
    int32_t *n_corr, *n_its, *corr, *sets;
    orbfe_pnp_hypothesis *hyp;
    uint32_t *bits;
    orbfe_pnp_refined *refined;
    uint32_t *refined_bits;
    int32_t *events, *n_events, *exhausted, *status;
    float *table; // [n_cands][PR_FIELDS][tcap]
    int32_t *records; // [n_cands][1 + max_its]: the number of record holders, then their iterations in ascending order
    float sigma2[ORBFE_MAX_LEVELS];
    float fx, fy, cx, cy, th2, epsilon;
    int32_t cap, tcap, words, nlevels, max_kf_n, min_inliers, max_its, n_iterations;
};

__device__ __forceinline__ PnPTable table_at(const float *tab, int stride)
{
    return PnPTable{tab, tab + stride, tab + 2 * (size_t)stride, tab + 3 * (size_t)stride, tab + 4 * (size_t)stride, tab + 5 * (size_t)stride};
}

__device__ __forceinline__ PnPCamera camera_of(const PnpArgs &a) { return PnPCamera{a.fx, a.fy, a.cx, a.cy}; }

__global__ __launch_bounds__(PR_THREADS) void pnp_filter_kernel(const PnpArgs a)
{
    __shared__ int s_wave[PR_THREADS / 64];
    __shared__ int s_invalid;
    const int c = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const orbfe_pnp_candidate rec = a.cands[c];
    if (threadIdx.x == 0) s_invalid = 0;
    const bool rec_ok = rec.n >= 0 && rec.n <= a.max_kf_n && rec.f_match && rec.pos && rec.valid && rec.draws;
    const int nk = rec_ok ? min(max(*a.n_keys, 0), a.cap) : 0;
    float *tab = a.table + (size_t)c * PR_FIELDS * a.tcap;
    int32_t *corr = a.corr + (size_t)c * 2 * a.cap;
    __syncthreads();
    int n_corr = 0;
    for (int i0 = 0; i0 < nk; i0 += PR_THREADS) {
        const int i = i0 + threadIdx.x;
        bool keep = false;
        int m = -1, oct = 0;
        if (i < nk) {
            m = rec.f_match[i];
            if (m != -1) {
                oct = a.keys[i].octave;
                if (m < -1 || m >= rec.n || oct < 0 || oct >= a.nlevels) s_invalid = 1; // checked before either becomes an address; every lane that writes writes this value
                else keep = rec.valid[m] != 0;
            }
        }
        const u64 vote = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(vote);
        __syncthreads();
        int before = n_corr, total = 0;
#pragma unroll
        for (int w = 0; w < PR_THREADS / 64; w++) {
            const int cw = s_wave[w];
            if (w < wave) before += cw;
            total += cw;
        }
        if (keep) {
            const int j = before + __popcll(vote & ((1ull << lane) - 1)); // < survivors so far <= i < cap <= tcap
            const float row[PR_FIELDS] = {rec.pos[3 * (size_t)m], rec.pos[3 * (size_t)m + 1], rec.pos[3 * (size_t)m + 2], a.keys[i].x, a.keys[i].y,
                                          __fmul_rn(a.sigma2[oct], a.th2)};
#pragma unroll
            for (int f = 0; f < PR_FIELDS; f++) tab[(size_t)f * a.tcap + j] = row[f];
            corr[2 * (size_t)j] = i; corr[2 * (size_t)j + 1] = m;
        }
        n_corr += total;
        __syncthreads(); // s_wave is rewritten by the next chunk; after the last one s_invalid is final
    }
    for (int j = n_corr + threadIdx.x; j < a.cap; j += PR_THREADS) { corr[2 * (size_t)j] = -1; corr[2 * (size_t)j + 1] = -1; }
    if (threadIdx.x == 0) {
        const int its = a.its_for_n[n_corr]; // n_corr <= nk <= cap
        // :183: `mnIterations < mRansacMaxIts || nCurrentIterations < nIterations`: the first call runs max(mRansacMaxIts, nIterations)
        a.n_its[c] = (its <= 0 || n_corr < 4) ? 0 : min(a.max_its, max(its, a.n_iterations));
        a.n_corr[c] = n_corr;
        a.status[c] = (!rec_ok || s_invalid) ? ORBFE_ERR_INVALID : 0;
    }
}

// CheckInliers of the wave over N correspondences with the pose P (R row-major, then t): the bit row, and the count (every lane's)
__device__ __forceinline__ int wave_check_inliers(const PnPTable &T, int N, const PnPCamera &cam, const double *P, uint32_t *row, int words, int lane)
{
    double R[3][3], t[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) R[i][j] = P[3 * i + j];
        t[i] = P[9 + i];
    }
    int count = 0;
    const int steps = (words + 1) >> 1;
    for (int st = 0; st < steps; st++) {
        const int j = st * 64 + lane;
        const bool inl = j < N && ORB_SLAM2::PnPIsInlier(T, j, cam, R, t);
        const u64 vote = __ballot(inl);
        count += __popcll(vote);
        if (lane < 2 && 2 * st + lane < words) row[2 * st + lane] = (uint32_t)(vote >> (32 * lane));
    }
    return count;
}

__global__ __launch_bounds__(64) void pnp_hyp_kernel(const PnpArgs a, const int lds_slots)
{
    extern __shared__ __attribute__((aligned(16))) double s_dyn[]; // [PR_HPW][12] poses, then the table [PR_FIELDS][lds_slots]
    double *s_pose = s_dyn;
    const int c = blockIdx.y, k0 = blockIdx.x * PR_HPW, lane = threadIdx.x;
    const int N = a.n_corr[c], n_its = a.n_its[c]; // written by pnp_filter_kernel: 0 <= N <= cap <= tcap
    const float *tab = a.table + (size_t)c * PR_FIELDS * a.tcap;
    int stride = a.tcap;
    if (N <= lds_slots && k0 < n_its) { // wave-uniform
        float *s_tab = (float *)(s_dyn + PR_HPW * 12);
        for (int f = 0; f < PR_FIELDS; f++)
            for (int j = lane; j < N; j += 64) s_tab[f * lds_slots + j] = tab[(size_t)f * a.tcap + j];
        tab = s_tab;
        stride = lds_slots;
    }
    __syncthreads();
    const PnPTable T = table_at(tab, stride);
    const PnPCamera cam = camera_of(a);
    orbfe_pnp_hypothesis *hyp = a.hyp + (size_t)c * a.max_its;
    uint32_t *bits = a.bits + (size_t)c * a.max_its * a.words;
    const int k = k0 + lane;
    double R[3][3], t[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) R[i][j] = 0.0;
        t[i] = 0.0;
    }
    if (lane < PR_HPW && k < a.max_its) {
        int32_t ids[4] = {-1, -1, -1, -1};
        if (k < n_its) { // N >= 4 here
            ORB_SLAM2::PnPDrawSet(a.cands[c].draws + 4 * (size_t)k, N, ids);
            const PnPSet S = {ids, nullptr, 4, 4};
            PnPWork w;
            ORB_SLAM2::PnPComputePose(T, S, cam, w, R, t);
#pragma unroll
            for (int i = 0; i < 3; i++) {
#pragma unroll
                for (int j = 0; j < 3; j++) s_pose[lane * 12 + 3 * i + j] = R[i][j];
                s_pose[lane * 12 + 9 + i] = t[i];
            }
        }
        if (a.sets) {
            int32_t *sets = a.sets + ((size_t)c * a.max_its + k) * 4;
            sets[0] = ids[0]; sets[1] = ids[1]; sets[2] = ids[2]; sets[3] = ids[3];
        }
    }
    __syncthreads();
    int my_count = 0;
    for (int hq = 0; hq < PR_HPW; hq++) {
        const int kq = k0 + hq; // wave-uniform
        if (kq >= a.max_its) break;
        uint32_t *row = bits + (size_t)kq * a.words;
        // the refinement rows of this iteration start as zeros; pnp_refine_kernel, two launches on, overwrites the record holders'
        uint32_t *rrow = a.refined_bits + ((size_t)c * a.max_its + kq) * a.words;
        for (int w = lane; w < a.words; w += 64) rrow[w] = 0u;
        if (lane < 16) ((uint32_t *)(a.refined + (size_t)c * a.max_its + kq))[lane] = 0u;
        if (kq >= n_its) {
            for (int w = lane; w < a.words; w += 64) row[w] = 0u;
            continue;
        }
        const int count = wave_check_inliers(T, N, cam, s_pose + hq * 12, row, a.words, lane);
        if (lane == hq) my_count = count;
    }
    if (lane < PR_HPW && k < a.max_its) { // the record: 64 bytes, zero from n_its on; best_k is pnp_scan_kernel's
        uint32_t rec[16];
        rec[0] = (uint32_t)my_count;
        rec[1] = (uint32_t)-1;
#pragma unroll
        for (int i = 0; i < 9; i++) rec[2 + i] = k < n_its ? __float_as_uint(one_nan((float)R[i / 3][i % 3])) : 0u;
#pragma unroll
        for (int i = 0; i < 3; i++) rec[11 + i] = k < n_its ? __float_as_uint(one_nan((float)t[i])) : 0u;
        rec[14] = 0u; rec[15] = 0u;
        uint32_t *out = (uint32_t *)(hyp + k); // the caller's array need only be 4-byte aligned
#pragma unroll
        for (int q = 0; q < 16; q++) out[q] = rec[q];
    }
}

__global__ __launch_bounds__(64) void pnp_scan_kernel(const PnpArgs a)
{
    const int c = blockIdx.x;
    if (threadIdx.x != 0) return;
    const int n_its = a.n_its[c], min_c = ORB_SLAM2::PnPMinInliers(a.n_corr[c], a.min_inliers, a.epsilon);
    int32_t *hyp = (int32_t *)(a.hyp + (size_t)c * a.max_its);
    int32_t *records = a.records + (size_t)c * (1 + a.max_its);
    int best = 0, best_k = -1, n_rec = 0; // mnBestInliers starts at 0
    for (int k = 0; k < n_its; k++) {
        const int count = hyp[16 * (size_t)k];
        if (count >= min_c && count > best) { best = count; best_k = k; records[1 + n_rec++] = k; } // n_rec <= k < max_its
        hyp[16 * (size_t)k + 1] = best_k;
    }
    records[0] = n_rec;
}

__global__ __launch_bounds__(64) void pnp_refine_kernel(const PnpArgs a)
{
    __shared__ double s_pose[12];
    const int c = blockIdx.y, lane = threadIdx.x;
    const int N = a.n_corr[c];
    const int32_t *records = a.records + (size_t)c * (1 + a.max_its);
    const int n_rec = min(max(records[0], 0), a.max_its);
    const PnPTable T = table_at(a.table + (size_t)c * PR_FIELDS * a.tcap, a.tcap);
    const PnPCamera cam = camera_of(a);
    for (int r = blockIdx.x; r < n_rec; r += PR_REFINE_WAVES) { // wave-uniform
        const int k = min(max(records[1 + r], 0), a.max_its - 1);
        const int32_t *hyp = (const int32_t *)(a.hyp + (size_t)c * a.max_its + k);
        uint32_t *out = (uint32_t *)(a.refined + (size_t)c * a.max_its + k);
        uint32_t *row = a.refined_bits + ((size_t)c * a.max_its + k) * a.words;
        if (lane == 0) {
            const PnPSet S = {nullptr, a.bits + ((size_t)c * a.max_its + k) * a.words, N, hyp[0]};
            PnPWork w;
            double R[3][3], t[3];
            ORB_SLAM2::PnPComputePose(T, S, cam, w, R, t);
            for (int i = 0; i < 3; i++) {
                for (int j = 0; j < 3; j++) s_pose[3 * i + j] = R[i][j];
                s_pose[9 + i] = t[i];
            }
        }
        __syncthreads();
        const int count = wave_check_inliers(T, N, cam, s_pose, row, a.words, lane);
        if (lane < 16) {
            uint32_t v = 0u;
            if (lane == 0) v = count > ORB_SLAM2::PnPMinInliers(N, a.min_inliers, a.epsilon) ? 1u : 0u;
            else if (lane == 1) v = (uint32_t)count;
            else if (lane < 14) {
                const int q = lane - 2, rr = q >> 2, cc = q & 3; // Tcw[3][4]
                v = __float_as_uint(one_nan((float)(cc < 3 ? s_pose[3 * rr + cc] : s_pose[9 + rr])));
            }
            out[lane] = v;
        }
        __syncthreads(); // s_pose is rewritten by the wave's next record holder
    }
}

__global__ __launch_bounds__(64) void pnp_events_kernel(const PnpArgs a)
{
    const int c = blockIdx.x, lane = threadIdx.x;
    __shared__ int s_nev;
    const int n_its = a.n_its[c];
    int32_t *events = a.events + (size_t)c * a.max_its;
    if (lane == 0) {
        const int min_c = ORB_SLAM2::PnPMinInliers(a.n_corr[c], a.min_inliers, a.epsilon);
        const int32_t *hyp = (const int32_t *)(a.hyp + (size_t)c * a.max_its);
        const int32_t *refined = (const int32_t *)(a.refined + (size_t)c * a.max_its);
        int nev = 0;
        for (int k = 0; k < n_its; k++) {
            const int count = hyp[16 * (size_t)k], b = hyp[16 * (size_t)k + 1]; // b <= k < n_its
            if (count >= min_c && b >= 0 && refined[16 * (size_t)b] != 0) events[nev++] = k;
        }
        s_nev = nev;
        a.n_events[c] = nev;
        a.exhausted[c] = n_its > 0 ? hyp[16 * (size_t)(n_its - 1) + 1] : -1;
    }
    __syncthreads();
    for (int e = s_nev + lane; e < a.max_its; e += 64) events[e] = -1;
}

struct SelectArgs {
    const int32_t *n_keys, *n_corr, *n_its, *corr, *exhausted;
    const orbfe_pnp_hypothesis *hyp;
    const orbfe_pnp_refined *refined;
    const uint32_t *bits, *refined_bits;
    float *Tcw;
    int32_t *cur_point, *status;
    uint8_t *has_point;
    int32_t c, which, k, cap, max_its, words;
};

__global__ __launch_bounds__(PR_THREADS) void pnp_select_kernel(const SelectArgs a)
{
    __shared__ int s_invalid;
    const int nk = min(max(*a.n_keys, 0), a.cap);
    const int N = min(max(a.n_corr[a.c], 0), a.cap), n_its = min(max(a.n_its[a.c], 0), a.max_its);
    const int32_t *hyp = (const int32_t *)(a.hyp + (size_t)a.c * a.max_its);
    const int32_t *refined = (const int32_t *)(a.refined + (size_t)a.c * a.max_its);
    int b = -1;
    const float *R = nullptr, *t = nullptr;
    int rs = 3, ts = 1;
    const uint32_t *row = nullptr;
    if (a.which == ORBFE_PNP_EVENT) {
        if (a.k < n_its) {
            b = hyp[16 * (size_t)a.k + 1];
            if (b < 0 || b >= n_its || refined[16 * (size_t)b] == 0) b = -1;
        }
        if (b >= 0) {
            R = (const float *)(refined + 16 * (size_t)b + 2); t = R + 3; rs = 4; ts = 4;
            row = a.refined_bits + ((size_t)a.c * a.max_its + b) * a.words;
        }
    } else {
        b = a.exhausted[a.c];
        if (b < 0 || b >= n_its) b = -1;
        if (b >= 0) {
            R = (const float *)(hyp + 16 * (size_t)b + 2); t = R + 9;
            row = a.bits + ((size_t)a.c * a.max_its + b) * a.words;
        }
    }
    if (threadIdx.x == 0) s_invalid = b < 0 ? 1 : 0;
    if (threadIdx.x < 16) {
        const int r = threadIdx.x >> 2, cc = threadIdx.x & 3;
        float v = r == cc ? 1.f : 0.f;
        if (b >= 0 && r < 3) v = cc < 3 ? R[rs * r + cc] : t[ts * r];
        a.Tcw[threadIdx.x] = v;
    }
    for (int i = threadIdx.x; i < nk; i += PR_THREADS) { a.cur_point[i] = -1; a.has_point[i] = 0; }
    __syncthreads();
    if (b >= 0) {
        const int32_t *corr = a.corr + (size_t)a.c * 2 * a.cap;
        for (int j = threadIdx.x; j < N; j += PR_THREADS)
            if ((row[j >> 5] >> (j & 31)) & 1u) {
                const int i = corr[2 * (size_t)j], m = corr[2 * (size_t)j + 1];
                if (i < 0 || i >= nk) { s_invalid = 1; continue; } // checked before it becomes an address
                a.cur_point[i] = m; // the keypoints of the correspondences ascend strictly: one writer per slot
                a.has_point[i] = 1;
            }
    }
    __syncthreads();
    if (threadIdx.x == 0) *a.status = s_invalid ? ORBFE_ERR_INVALID : 0;
}

bool finite_nonneg(float v) { return v >= 0.f && v <= 3.4e38f; }

// the five launches on frame (keys, d_n_keys, cap); the arguments have been checked
int enqueue_impl(orbfe_context *ctx, hipStream_t s, const KeyPointPOD *keys, const int32_t *d_n_keys, int cap, const orbfe_pnp_candidate *d_cands, int n_cands,
                 int max_kf_n, int min_inliers, int max_its, int n_iterations, float epsilon, float th2, const int32_t *d_its_for_n, int32_t *d_n_corr,
                 int32_t *d_n_its, int32_t *d_corr, int32_t *d_sets, orbfe_pnp_hypothesis *d_hyp, uint32_t *d_inlier_bits, orbfe_pnp_refined *d_refined,
                 uint32_t *d_refined_bits, int32_t *d_events, int32_t *d_n_events, int32_t *d_exhausted, int32_t *d_status)
{
    const orbfe_params *cp = &ctx->params;
    PnpArgs a;
    a.keys = keys; a.n_keys = d_n_keys; a.cands = d_cands; a.its_for_n = d_its_for_n;
    a.n_corr = d_n_corr; a.n_its = d_n_its; a.corr = d_corr; a.sets = d_sets; a.hyp = d_hyp; a.bits = d_inlier_bits; a.refined = d_refined;
    a.refined_bits = d_refined_bits; a.events = d_events; a.n_events = d_n_events; a.exhausted = d_exhausted; a.status = d_status;
    for (int l = 0; l < ORBFE_MAX_LEVELS; l++) a.sigma2[l] = l < cp->nlevels ? ctx->plan.sigma2[l] : 0.f;
    a.fx = cp->fx; a.fy = cp->fy; a.cx = cp->cx; a.cy = cp->cy; a.th2 = th2; a.epsilon = epsilon;
    a.cap = cap; a.tcap = (cap + 3) & ~3; a.words = (cap + 31) / 32;
    a.nlevels = cp->nlevels; a.max_kf_n = max_kf_n; a.min_inliers = min_inliers; a.max_its = max_its; a.n_iterations = n_iterations;
    const size_t table_bytes = sizeof(float) * PR_FIELDS * (size_t)a.tcap * n_cands; // tcap is a multiple of 4: the records behind it are aligned
    if (ctx->pnp_ransac_scratch.ensure(table_bytes + sizeof(int32_t) * (1 + (size_t)max_its) * n_cands)) return orbfe_fail(ctx, ORBFE_ERR_HIP, "PnP RANSAC scratch allocation failed");
    a.table = (float *)ctx->pnp_ransac_scratch.p;
    a.records = (int32_t *)((uint8_t *)ctx->pnp_ransac_scratch.p + table_bytes);
    const int lds_slots = std::min(a.tcap, ORBFE_PNP_RANSAC_LDS_SLOTS);
    const size_t lds = sizeof(double) * PR_HPW * 12 + sizeof(float) * PR_FIELDS * (size_t)lds_slots;
    hipLaunchKernelGGL(pnp_filter_kernel, dim3(n_cands), dim3(PR_THREADS), 0, s, a);
    hipLaunchKernelGGL(pnp_hyp_kernel, dim3((max_its + PR_HPW - 1) / PR_HPW, n_cands), dim3(64), lds, s, a, lds_slots);
    hipLaunchKernelGGL(pnp_scan_kernel, dim3(n_cands), dim3(64), 0, s, a);
    hipLaunchKernelGGL(pnp_refine_kernel, dim3(PR_REFINE_WAVES, n_cands), dim3(64), 0, s, a);
    hipLaunchKernelGGL(pnp_events_kernel, dim3(n_cands), dim3(64), 0, s, a);
    ORBFE_HIP_TRY(ctx, hipGetLastError());
    return ORBFE_OK;
}

int check_batch_args(orbfe_context *ctx, int n_cands, int max_kf_n, int min_set, int min_inliers, int max_its, int n_iterations, float epsilon, float th2)
{
    if (n_cands < 0 || n_cands > 65535) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "n_cands = %d (0 .. 65535)", n_cands);
    if (max_kf_n < 0 || max_kf_n > 65535) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "max_kf_n = %d (0 .. 65535)", max_kf_n);
    if (min_set != 4) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "min_set = %d: EPnP hypotheses draw four correspondences (mRansacMinSet of Tracking)", min_set);
    if (min_inliers < 1) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "min_inliers = %d", min_inliers);
    if (max_its < 1 || max_its > 65536 || n_iterations < 0) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "max_its = %d (1 .. 65536), n_iterations = %d (>= 0)", max_its, n_iterations);
    if (!finite_nonneg(epsilon) || !finite_nonneg(th2)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "epsilon and th2 must be finite and not negative");
    const orbfe_params *cp = &ctx->params;
    if (cp->nlevels < 1 || cp->nlevels > ORBFE_MAX_LEVELS) return orbfe_fail(ctx, ORBFE_ERR_UNSUPPORTED, "nlevels = %d", cp->nlevels);
    return ORBFE_OK;
}

} // namespace

extern "C" int orbfe_enqueue_pnp_ransac_batch(orbfe_context *ctx, int slot, const orbfe_pnp_candidate *d_cands, int n_cands, int max_kf_n, int min_set,
                                              int min_inliers, int max_its, int n_iterations, float epsilon, float th2, const int32_t *d_its_for_n,
                                              int32_t *d_n_corr, int32_t *d_n_its, int32_t *d_corr, int32_t *d_sets, orbfe_pnp_hypothesis *d_hyp,
                                              uint32_t *d_inlier_bits, orbfe_pnp_refined *d_refined, uint32_t *d_refined_bits, int32_t *d_events,
                                              int32_t *d_n_events, int32_t *d_exhausted, int32_t *d_status, void *stream)
try {
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    ORBFE_ENTRY(ctx);
    if (!d_n_corr || !d_n_its || !d_corr || !d_hyp || !d_inlier_bits || !d_refined || !d_refined_bits || !d_events || !d_n_events || !d_exhausted || !d_status)
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null argument");
    if (const int rc = check_batch_args(ctx, n_cands, max_kf_n, min_set, min_inliers, max_its, n_iterations, epsilon, th2)) return rc;
    if (n_cands > 0 && (!d_cands || !d_its_for_n)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null candidate array or iteration table");
    if (slot < 0 || slot >= ctx->last_images) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "device slot %d: the latest extraction call filled %d image slots", slot, ctx->last_images);
    if (n_cands == 0) return ORBFE_OK;
    const orbfe_keypoint *keys = nullptr;
    if (const int rc = orbfe_device_keys_un(ctx, slot, &keys, stream)) return rc; // mvKeysUn; orders the stream behind the extraction
    hipStream_t s;
    if (const int rc = orbfe_enqueue_on(ctx, stream, true, &s)) return rc;
    return enqueue_impl(ctx, s, (const KeyPointPOD *)keys, ctx->buf.kp_cnt + slot, ctx->cfg.sel_total, d_cands, n_cands, max_kf_n, min_inliers, max_its, n_iterations,
                        epsilon, th2, d_its_for_n, d_n_corr, d_n_its, d_corr, d_sets, d_hyp, d_inlier_bits, d_refined, d_refined_bits, d_events, d_n_events,
                        d_exhausted, d_status);
} ORBFE_CATCH(ctx)

extern "C" int orbfe_enqueue_pnp_ransac_select(orbfe_context *ctx, int slot, int n_cands, int c, int which, int k, int max_its, const int32_t *d_n_corr,
                                               const int32_t *d_n_its, const int32_t *d_corr, const orbfe_pnp_hypothesis *d_hyp, const uint32_t *d_inlier_bits,
                                               const orbfe_pnp_refined *d_refined, const uint32_t *d_refined_bits, const int32_t *d_exhausted, float *d_Tcw_row,
                                               int32_t *d_cur_point_row, uint8_t *d_has_point_row, int32_t *d_status, void *stream)
try {
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    ORBFE_ENTRY(ctx);
    if (!d_n_corr || !d_n_its || !d_corr || !d_hyp || !d_inlier_bits || !d_refined || !d_refined_bits || !d_exhausted || !d_Tcw_row || !d_cur_point_row ||
        !d_has_point_row || !d_status)
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null argument");
    if (slot < 0 || slot >= ctx->last_images) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "device slot %d: the latest extraction call filled %d image slots", slot, ctx->last_images);
    if (which != ORBFE_PNP_EVENT && which != ORBFE_PNP_EXHAUSTED) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "which = %d", which);
    if (max_its < 1 || max_its > 65536 || c < 0 || c >= n_cands || (which == ORBFE_PNP_EVENT && (k < 0 || k >= max_its)))
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "candidate %d of %d, iteration %d of %d", c, n_cands, k, max_its);
    hipStream_t s;
    if (const int rc = orbfe_enqueue_on(ctx, stream, true, &s)) return rc;
    SelectArgs a;
    a.n_keys = ctx->buf.kp_cnt + slot; a.n_corr = d_n_corr; a.n_its = d_n_its; a.corr = d_corr; a.exhausted = d_exhausted; a.hyp = d_hyp; a.refined = d_refined;
    a.bits = d_inlier_bits; a.refined_bits = d_refined_bits; a.Tcw = d_Tcw_row; a.cur_point = d_cur_point_row; a.status = d_status; a.has_point = d_has_point_row;
    a.c = c; a.which = which; a.k = which == ORBFE_PNP_EVENT ? k : 0; a.cap = ctx->cfg.sel_total; a.max_its = max_its; a.words = (a.cap + 31) / 32;
    hipLaunchKernelGGL(pnp_select_kernel, dim3(1), dim3(PR_THREADS), 0, s, a);
    ORBFE_HIP_TRY(ctx, hipGetLastError());
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

extern "C" int orbfe_pnp_ransac(orbfe_context *ctx, const orbfe_keypoint *keys_un, int n_keys, const int32_t *f_match, const float *pos, const int32_t *valid,
                                int n_kf, const uint32_t *draws, int min_set, int min_inliers, int max_its, int n_iterations, float epsilon, float th2,
                                const int32_t *its_for_n, int *n_corr, int *n_its, int32_t *corr, int32_t *sets, orbfe_pnp_hypothesis *hyp, uint32_t *inlier_bits,
                                orbfe_pnp_refined *refined, uint32_t *refined_bits, int32_t *events, int *n_events, int *exhausted)
try {
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    ORBFE_ENTRY(ctx);
    if (!draws || !its_for_n || !n_corr || !n_its || !corr || !hyp || !inlier_bits || !refined || !refined_bits || !events || !n_events || !exhausted)
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null argument");
    if (n_keys < 0 || n_keys > 65535 || n_kf < 0 || n_kf > 65535) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "%d keypoints, %d keyframe slots (0 .. 65535)", n_keys, n_kf);
    if (n_keys > 0 && (!keys_un || !f_match)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null array of the frame");
    if (n_kf > 0 && (!pos || !valid)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null array of the keyframe");
    if (const int rc = check_batch_args(ctx, 1, n_kf, min_set, min_inliers, max_its, n_iterations, epsilon, th2)) return rc;
    hipStream_t s;
    if (const int rc = orbfe_enqueue_on(ctx, nullptr, false, &s)) return rc;
    const int cap = std::max(n_keys, 1), words = (cap + 31) / 32;
    // the staging block: results first, then the inputs
    const size_t its = (size_t)max_its;
    orbfe::StageLayout L;
    const auto f_cnt = L.result<int32_t>(8); // n_corr, n_its, n_events, exhausted, status
    const auto f_corr = L.result<int32_t>(cap, 2); const auto f_sets = L.result<int32_t>(its, 4); const auto f_hyp = L.result<orbfe_pnp_hypothesis>(its);
    const auto f_bits = L.result<uint32_t>(its, words); const auto f_ref = L.result<orbfe_pnp_refined>(its); const auto f_rbits = L.result<uint32_t>(its, words);
    const auto f_ev = L.result<int32_t>(its);
    const auto f_rec = L.input<orbfe_pnp_candidate>(1); const auto f_nk = L.input<int32_t>(1);
    const auto f_keys = L.input<KeyPointPOD>(n_keys); const auto f_fm = L.input<int32_t>(n_keys); const auto f_pos = L.input<float>(n_kf, 3);
    const auto f_val = L.input<int32_t>(n_kf); const auto f_draws = L.input<uint32_t>(its, 4); const auto f_tab = L.input<int32_t>((size_t)cap + 1);
    if (ctx->sync_stage.ensure(L.bytes())) return orbfe_fail(ctx, ORBFE_ERR_HIP, "PnP RANSAC staging allocation failed");
    StageBlock blk(L, ctx->sync_stage);
    blk.put(f_keys, keys_un, n_keys); blk.put(f_fm, f_match, n_keys); blk.put(f_pos, pos, 3 * (size_t)n_kf); blk.put(f_val, valid, n_kf);
    blk.put(f_draws, draws, 4 * its); blk.put(f_tab, its_for_n, (size_t)n_keys + 1); // the table covers N <= n_keys
    const int32_t nk32 = n_keys;
    blk.put(f_nk, &nk32, 1);
    orbfe_pnp_candidate rec = {};
    rec.f_match = blk.dev(f_fm); rec.pos = blk.dev(f_pos); rec.valid = blk.dev(f_val); rec.draws = blk.dev(f_draws); rec.n = n_kf;
    blk.put(f_rec, &rec, 1);
    ORBFE_HIP_TRY(ctx, blk.upload(s));
    int32_t *cnt = blk.dev(f_cnt);
    const int rc = enqueue_impl(ctx, s, blk.dev(f_keys), blk.dev(f_nk), cap, blk.dev(f_rec), 1, n_kf, min_inliers, max_its, n_iterations, epsilon, th2, blk.dev(f_tab), cnt,
                                cnt + 1, blk.dev(f_corr), blk.dev(f_sets), blk.dev(f_hyp), blk.dev(f_bits), blk.dev(f_ref), blk.dev(f_rbits), blk.dev(f_ev), cnt + 2,
                                cnt + 3, cnt + 4);
    if (rc != ORBFE_OK) return rc;
    ORBFE_HIP_TRY(ctx, blk.download(s));
    ORBFE_HIP_TRY(ctx, hipStreamSynchronize(s));
    int32_t c5[5];
    blk.get(f_cnt, c5, 5);
    *n_corr = c5[0]; *n_its = c5[1]; *n_events = c5[2]; *exhausted = c5[3];
    blk.get(f_corr, corr, f_corr.count);
    if (sets) blk.get(f_sets, sets, f_sets.count);
    blk.get(f_hyp, hyp, f_hyp.count); blk.get(f_bits, inlier_bits, f_bits.count); blk.get(f_ref, refined, f_ref.count); blk.get(f_rbits, refined_bits, f_rbits.count);
    blk.get(f_ev, events, f_ev.count);
    if (c5[4] != 0) return orbfe_fail(ctx, c5[4], "a match index out of range or a keypoint octave outside the context's %d levels", ctx->params.nlevels);
    return ORBFE_OK;
} ORBFE_CATCH(ctx)
