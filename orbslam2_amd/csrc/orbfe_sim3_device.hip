// orbfe_sim3_device.hip -- ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (src/ORBmatcher.cc:1098-1322) of
// LoopClosing::ComputeSim3 (src/LoopClosing.cc:359) on two device-resident keyframes, asynchronous on the caller's stream.  Device
// pointers in, vpMatches12 in HBM, no host wait.
//
// orbfe_search_by_sim3 (orbfe_match.hip) is the synchronous form and the second implementation this one is tested against: there every
// point is projected on the host, each keyframe is uploaded and bucketed per call and direction, and the candidate list of every window
// comes back over the link.  ComputeSim3 calls the matcher for the same current keyframe once per candidate and RANSAC round; here the
// keyframes are orbfe_grid_keyframe records whose arrays and grid stay in HBM.  The points do not interact, so the search is
//   sim3_one_way_kernel   both directions in one launch (blockIdx.y), one wave per keypoint slot of the source keyframe: the point's
//                         window query against the target's View (query_sim3_point, orbfe_match_resolve.h: the very text the
//                         synchronous call runs on the host), then wave_best_key without a gate (orbfe_match_window.hpp):
//                         GetFeaturesInArea over the target's own grid, the smallest candidate key of the wave = the reference loop's
//                         first minimum, accepted at <= TH_HIGH
//   sim3_agree_kernel     one thread per keypoint of KF1: the agreement check of :1293-1308, d_match12 and the count
// behind sim3_reset_kernel, which clears the count and the status.  The one-way results live in the context's matcher scratch.
// The grids and keypoints are the caller's uploads, so the walk is the CHECKED one, as in orbfe_fuse_device.hip.
#include "../../include/orbfe.h"
#include "orbfe_device.h"
#include "orbfe_host.h"
#include "orbfe_match_resolve.h"
#include "orbfe_match_window.hpp"

#include <algorithm>

using orbfe_resolve::key_dist;
using orbfe_resolve::key_idx;
using orbfe_resolve::MatchQuery;
using orbfe_resolve::TH_HIGH;
using orbfe_resolve::View;

int32_t *orbfe_ctx_sim3_scratch(orbfe_context *ctx, size_t n); // orbfe_match_device.hip

struct Sim3Side { // one direction: the map points of keyframe A, one per keypoint slot, searched in keyframe B
    GridFrame f;            // B: n_ptr null, cap = its keypoint count
    View V;                 // with B's bounds
    float Taw[12], sRt[12]; // world -> camera A, and [sR|t] from there into camera B
    int n;                  // keypoint slots of A
    const float *pos, *max_distance, *min_distance;
    const uint8_t *desc;
    const int32_t *valid;
    int32_t *match; // [n]: keypoint of B or -1
};
struct Sim3Args {
    Sim3Side side[2]; // 0: KF1's points in KF2 (:1143-1216), 1: KF2's points in KF1 (:1218-1291)
    float th;
    int32_t *status;
};

__global__ __launch_bounds__(64) void sim3_reset_kernel(int32_t *n_found, int32_t *status)
{
    if (threadIdx.x == 0) { *n_found = 0; *status = 0; }
}

__global__ __launch_bounds__(256) void sim3_one_way_kernel(Sim3Args a)
{
    const Sim3Side &S = a.side[blockIdx.y];
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6); // wave-uniform: every branch on i or n below is taken by whole waves
    const int lane = threadIdx.x & 63;
    if (i >= S.n) return;
    const int n = S.f.cap;
    bool clean = true;
    unsigned long long best = NO_KEY;
    if (n > 0) { // a target without keypoints has no window, and none of its arrays (or the points') is read
        MatchQuery Q = {0, 0, 0, 0, -1, 0, 0, 0};
        const float p[3] = {S.pos[3 * (size_t)i], S.pos[3 * (size_t)i + 1], S.pos[3 * (size_t)i + 2]};
        orbfe_resolve::query_sim3_point(S.V, S.Taw, S.sRt, p, S.valid[i], S.max_distance[i], S.min_distance[i], a.th, Q);
        best = wave_best_key(S.f, Q, S.desc + (size_t)i * 32, lane, [](int, const KeyPointPOD &) { return true; }, n, S.V.nlevels, clean);
    }
    if (lane == 0) {
        S.match[i] = (best != NO_KEY && key_dist(best) <= TH_HIGH) ? key_idx(best) : -1; // in [0, n): the checked walk has tested it
        if (!clean) *a.status = ORBFE_ERR_INVALID; // every wave that writes writes this value
    }
}

// check agreement (:1293-1308): KF1 keypoint i1 keeps its KF2 keypoint when that one's point came back to i1
__global__ __launch_bounds__(256) void sim3_agree_kernel(int n1, const int32_t *__restrict__ m1, const int32_t *__restrict__ m2, int32_t *__restrict__ match12,
                                                         int32_t *n_found)
{
    const int i1 = blockIdx.x * 256 + threadIdx.x;
    bool ok = false;
    if (i1 < n1) {
        const int idx2 = m1[i1]; // -1, or a keypoint of KF2: m2 has an entry for it
        ok = idx2 >= 0 && m2[idx2] == i1;
        match12[i1] = ok ? idx2 : -1;
    }
    const int cnt = __popcll(__ballot(ok));
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(n_found, cnt); // an integer count: the order of the waves does not matter
}


static void sim3_side(orbfe_context *ctx, Sim3Side &S, const orbfe_grid_keyframe *kfb, const float *Taw, const float *sRt, int n, const float *d_pos, const float *d_max_distance,
                      const float *d_min_distance, const uint8_t *d_desc, const int32_t *d_valid, int32_t *d_match)
{
    S.f.u_right = nullptr; // SearchBySim3 has no mvuRight gate: the record's u_right is never read
    S.V = orbfe_view(ctx, kfb);
    for (int k = 0; k < 12; k++) { S.Taw[k] = Taw[k]; S.sRt[k] = sRt[k]; }
    S.n = n;
    S.pos = d_pos; S.max_distance = d_max_distance; S.min_distance = d_min_distance; S.desc = d_desc; S.valid = d_valid;
    S.match = d_match;
}

extern "C" int orbfe_enqueue_search_by_sim3(orbfe_context *ctx, const orbfe_grid_keyframe *kf1, const float *T1w, const float *d_pos1,
                                            const float *d_max_distance1, const float *d_min_distance1, const uint8_t *d_pt_desc1, const int32_t *d_valid1,
                                            const orbfe_grid_keyframe *kf2, const float *T2w, const float *d_pos2, const float *d_max_distance2,
                                            const float *d_min_distance2, const uint8_t *d_pt_desc2, const int32_t *d_valid2, float s12, const float *R12,
                                            const float *t12, float th, int32_t *d_match12, int32_t *d_n_found, int32_t *d_status, void *stream)
try {
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    ORBFE_ENTRY(ctx);
    if (!kf1 || !kf2 || !T1w || !T2w || !R12 || !t12 || !d_match12 || !d_n_found || !d_status) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null argument");
    Sim3Args a;
    int rc = orbfe_grid_frame_of_record(ctx, kf2, a.side[0].f); // KF1's points are searched in KF2 ...
    if (rc != ORBFE_OK) return rc;
    rc = orbfe_grid_frame_of_record(ctx, kf1, a.side[1].f); // ... and KF2's in KF1
    if (rc != ORBFE_OK) return rc;
    const int n1 = kf1->n, n2 = kf2->n;
    if (n1 > 0 && n2 > 0 &&
        (!d_pos1 || !d_max_distance1 || !d_min_distance1 || !d_pt_desc1 || !d_valid1 || !d_pos2 || !d_max_distance2 || !d_min_distance2 || !d_pt_desc2 ||
         !d_valid2 || !kf1->keys_un || !kf1->desc || !kf1->cell_off || !kf1->cell_idx || !kf2->keys_un || !kf2->desc || !kf2->cell_off || !kf2->cell_idx))
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null array among the map points or in a keyframe record");
    const orbfe_params *P = &ctx->params;
    if (P->nlevels < 1 || P->nlevels > ORBFE_MAX_LEVELS) return orbfe_fail(ctx, ORBFE_ERR_UNSUPPORTED, "nlevels = %d", P->nlevels);
    hipStream_t s;
    rc = orbfe_enqueue_on(ctx, stream, false, &s);
    if (rc != ORBFE_OK) return rc;
    int32_t *m = orbfe_ctx_sim3_scratch(ctx, (size_t)n1 + (size_t)n2);
    if (!m) return orbfe_fail(ctx, ORBFE_ERR_HIP, "matcher scratch allocation failed");
    hipLaunchKernelGGL(sim3_reset_kernel, dim3(1), dim3(64), 0, s, d_n_found, d_status);
    if (n1 > 0) { // without keypoints in KF1 there is no d_match12 entry to write; without any in KF2 every entry is -1 and no array is read
        float A12[12], A21[12];
        orbfe_resolve::sim3_pair(s12, R12, t12, A12, A21);
        sim3_side(ctx, a.side[0], kf2, T1w, A21, n1, d_pos1, d_max_distance1, d_min_distance1, d_pt_desc1, d_valid1, m);
        sim3_side(ctx, a.side[1], kf1, T2w, A12, n2, d_pos2, d_max_distance2, d_min_distance2, d_pt_desc2, d_valid2, m + n1);
        a.th = th;
        a.status = d_status;
        hipLaunchKernelGGL(sim3_one_way_kernel, dim3((std::max(n1, n2) + 3) / 4, 2), dim3(256), 0, s, a);
        hipLaunchKernelGGL(sim3_agree_kernel, dim3((n1 + 255) / 256), dim3(256), 0, s, n1, m, m + n1, d_match12, d_n_found);
    }
    ORBFE_HIP_TRY(ctx, hipGetLastError());
    return ORBFE_OK;
} ORBFE_CATCH(ctx)
