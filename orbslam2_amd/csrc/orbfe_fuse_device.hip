// orbfe_fuse_device.hip -- the search half of ORBmatcher::Fuse on device-resident keyframes, asynchronous on the caller's stream:
// Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cc:821-971) of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:454-531) and
// Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (:973-1096) of LoopClosing::SearchAndFuse.  Device pointers in, best keypoint per query
// in HBM, no host wait.
//
// orbfe_fuse / orbfe_fuse_sim3 (orbfe_match.hip) are the synchronous forms and the second implementation this one is tested against:
// there every point is projected on the host, the keyframe is uploaded and bucketed per call, the candidate list of every window
// comes back over the link and the host applies the chi-square gates and takes the minimum.  Fuse has no greedy state -- the points
// do not interact, the map mutation stays with the caller -- so here the whole search is ONE kernel:
//   fuse_kernel   one wave per query: its row of the PointTable, the point's window query against the keyframe's View (query_fuse_point,
//                 orbfe_match_resolve.h: the very text the synchronous calls run on the host), then wave_best_key
//                 (orbfe_match_window.hpp): GetFeaturesInArea over the keyframe's own grid (lane j owns cells j, j + 64, ...), the
//                 chi-square gates per hit (fuse_chi2_passes, again the host's text), the smallest candidate key of the wave = the
//                 reference loop's first minimum; lane 0 writes best_idx and adds to the count
// behind fuse_reset_kernel, which clears the count and the status on the stream.  The keyframe's grid is built once per keyframe by
// grid_build_kernel (orbfe_enqueue_keyframe_grid) into arrays the caller keeps.  The calls own no scratch.
// The grid and the keypoints are the caller's uploads, so the walk is the CHECKED one: offsets, indices and octaves are tested
// before they become addresses, and what fails is reported in d_status.  What the calls refuse before a launch is
// orbfe_point_table_frame, which the Sim3 SearchByProjection (orbfe_match_device.hip) shares.
#include "../../include/orbfe.h"
#include "orbfe_device.h"
#include "orbfe_host.h"
#include "orbfe_match_resolve.h"
#include "orbfe_match_window.hpp"

#include <climits>

using orbfe_resolve::key_dist;
using orbfe_resolve::key_idx;
using orbfe_resolve::MatchQuery;
using orbfe_resolve::TH_LOW;
using orbfe_resolve::View;

static_assert(sizeof(orbfe_grid_keyframe) == 64, "orbfe_grid_keyframe: five pointers, four bounds and two counts");
static_assert(sizeof(orbfe_keypoint) == sizeof(KeyPointPOD), "the keyframe's keypoints are read as KeyPointPOD");

struct FuseArgs {
    GridFrame f;        // the keyframe: n_ptr null, cap = its keypoint count
    View V;             // with the keyframe's bounds
    float T[12], ow[3]; // [R|t] (of Tcw, or of the decomposed Scw) and the camera centre, both computed on the host
    int sim3;           // Fuse(pKF, Scw, ...): reciprocal of z in double, no chi-square gates
    int n_pts;
    PointTable pts;
    float th;
    int32_t *best_idx, *n_fused, *status;
};

__global__ __launch_bounds__(64) void fuse_reset_kernel(int32_t *n_fused, int32_t *status)
{
    if (threadIdx.x == 0) { *n_fused = 0; *status = 0; }
}

__global__ __launch_bounds__(256) void fuse_kernel(FuseArgs a)
{
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6); // wave-uniform: every branch on q, row or n below is taken by whole waves
    const int lane = threadIdx.x & 63;
    if (q >= a.n_pts) return;
    const int n = a.f.cap;
    const PointTable &t = a.pts;
    const int row = t.row(q); // -1: the index list names no row of the table, the query gets -1 and the call ORBFE_ERR_INVALID
    bool clean = true;
    unsigned long long best = NO_KEY;
    if (n > 0 && row >= 0) { // a keyframe without keypoints has no window, and none of its arrays (or the table's) is read
        MatchQuery Q = {0, 0, 0, 0, -1, 0, 0, 0};
        float ur = 0.f;
        const float p[3] = {t.pos[3 * (size_t)row], t.pos[3 * (size_t)row + 1], t.pos[3 * (size_t)row + 2]};
        const float nr[3] = {t.normal[3 * (size_t)row], t.normal[3 * (size_t)row + 1], t.normal[3 * (size_t)row + 2]};
        orbfe_resolve::query_fuse_point(a.V, a.T, a.ow, a.sim3, p, nr, t.pt_valid[q], t.max_distance[row], t.min_distance[row], a.th, Q, &ur);
        best = wave_best_key(
            a.f, Q, t.pt_desc + (size_t)row * 32, lane,
            [&](int idx, const KeyPointPOD &kp) {
                return a.sim3 || orbfe_resolve::fuse_chi2_passes(Q.u, Q.v, ur, kp.x, kp.y, a.f.u_right ? a.f.u_right[idx] : -1.f, a.V.sf[kp.octave]);
            },
            n, a.V.nlevels, clean);
    }
    const bool bad = row < 0 || !clean;
    if (lane == 0) {
        const int idx = (best != NO_KEY && key_dist(best) <= TH_LOW) ? key_idx(best) : -1;
        a.best_idx[q] = idx;
        if (idx >= 0) atomicAdd(a.n_fused, 1); // an integer count: the order of the waves does not matter
        if (bad) *a.status = ORBFE_ERR_INVALID; // every wave that writes writes this value
    }
}


// the part of a GridFrame that the grid builder and the window walk share: where the keypoints are and how cells are assigned
static int grid_frame_of(orbfe_context *ctx, const orbfe_keypoint *d_keys_un, int n, float min_x, float max_x, float min_y, float max_y, int keyframe,
                         const int32_t *d_cell_off, const int32_t *d_cell_idx, GridFrame &f)
{
    if (n < 0) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "negative keypoint count");
    if (n > 65535) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "keyframes with more than 65535 keypoints are not supported by the matchers");
    if (!(max_x > min_x) || !(max_y > min_y)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "bad image bounds");
    f.keys = (const KeyPointPOD *)d_keys_un;
    f.desc = nullptr; f.u_right = nullptr;
    f.n_ptr = nullptr; f.cap = n;
    grid_frame_geometry(f, min_x, max_x, min_y, max_y, keyframe != 0);
    f.cell_off = const_cast<int *>(d_cell_off); f.cell_idx = const_cast<int *>(d_cell_idx); // only grid_build_kernel writes them
    return ORBFE_OK;
}

// a keyframe record as the kernels read it (orbfe_match_device.hip and orbfe_sim3_device.hip build theirs here too)
int orbfe_grid_frame_of_record(orbfe_context *ctx, const orbfe_grid_keyframe *kf, GridFrame &f)
{
    const int rc = grid_frame_of(ctx, kf->keys_un, kf->n, kf->min_x, kf->max_x, kf->min_y, kf->max_y, kf->keyframe, kf->cell_off, kf->cell_idx, f);
    if (rc != ORBFE_OK) return rc;
    f.desc = kf->desc; f.u_right = kf->u_right;
    return ORBFE_OK;
}

extern "C" int orbfe_enqueue_keyframe_grid(orbfe_context *ctx, const orbfe_keypoint *d_keys_un, int n, const float *bounds, int32_t *d_cell_off,
                                           int32_t *d_cell_idx, void *stream)
try {
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    ORBFE_ENTRY(ctx);
    if (!bounds || !d_cell_off || (n > 0 && (!d_keys_un || !d_cell_idx))) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null argument");
    GridFrame f;
    int rc = grid_frame_of(ctx, d_keys_un, n, bounds[0], bounds[1], bounds[2], bounds[3], 0, d_cell_off, d_cell_idx, f);
    if (rc != ORBFE_OK) return rc;
    hipStream_t s;
    rc = orbfe_enqueue_on(ctx, stream, false, &s);
    if (rc != ORBFE_OK) return rc;
    orbfe_launch_grid_build(f, s); // with n == 0: 3073 zero offsets, no other access
    ORBFE_HIP_TRY(ctx, hipGetLastError());
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

int orbfe_point_table_frame(orbfe_context *ctx, const orbfe_grid_keyframe *kf, int n_pts, int max_pts, const PointTable &t, GridFrame &f)
{
    if (n_pts < 0 || t.n_rows < 0) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "negative count");
    if (!t.pt_index && t.n_rows < n_pts) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "%d queries without an index list over a table of %d rows", n_pts, t.n_rows);
    if (n_pts > max_pts) return orbfe_fail(ctx, ORBFE_ERR_CAPACITY, "%d points: the matcher's scratch rows hold %d", n_pts, max_pts);
    const int rc = orbfe_grid_frame_of_record(ctx, kf, f);
    if (rc != ORBFE_OK) return rc;
    if (n_pts > 0 && kf->n > 0 &&
        (!t.pos || !t.normal || !t.max_distance || !t.min_distance || !t.pt_desc || !t.pt_valid || !kf->keys_un || !kf->desc || !kf->cell_off || !kf->cell_idx))
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null array in the point table or in the keyframe record");
    const int nlevels = ctx->params.nlevels;
    if (nlevels < 1 || nlevels > ORBFE_MAX_LEVELS) return orbfe_fail(ctx, ORBFE_ERR_UNSUPPORTED, "nlevels = %d", nlevels);
    return ORBFE_OK;
}

static int enqueue_fuse(orbfe_context *ctx, int sim3, const orbfe_grid_keyframe *kf, const float *pose, int n_pts, const int32_t *d_pt_index, int n_rows,
                        const float *d_pos, const float *d_normal, const float *d_max_distance, const float *d_min_distance, const uint8_t *d_pt_desc,
                        const int32_t *d_pt_valid, float th, int32_t *d_best_idx, int32_t *d_n_fused, int32_t *d_status, void *stream)
{
    if (!kf || !pose || !d_best_idx || !d_n_fused || !d_status) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null argument");
    FuseArgs a;
    a.pts = {d_pt_index, n_rows, d_pos, d_normal, d_max_distance, d_min_distance, d_pt_desc, d_pt_valid};
    int rc = orbfe_point_table_frame(ctx, kf, n_pts, INT_MAX, a.pts, a.f); // the calls own no scratch: any count
    if (rc != ORBFE_OK) return rc;
    a.V = orbfe_view(ctx, kf);
    if (sim3) orbfe_resolve::sim3_to_rt(pose, a.T);
    else for (int k = 0; k < 12; k++) a.T[k] = pose[k];
    orbfe_resolve::camera_center(a.T, a.ow);
    a.sim3 = sim3;
    a.n_pts = n_pts;
    a.th = th;
    a.best_idx = d_best_idx; a.n_fused = d_n_fused; a.status = d_status;
    hipStream_t s;
    rc = orbfe_enqueue_on(ctx, stream, false, &s);
    if (rc != ORBFE_OK) return rc;
    hipLaunchKernelGGL(fuse_reset_kernel, dim3(1), dim3(64), 0, s, d_n_fused, d_status);
    if (n_pts > 0) hipLaunchKernelGGL(fuse_kernel, dim3((n_pts + 3) / 4), dim3(256), 0, s, a);
    ORBFE_HIP_TRY(ctx, hipGetLastError());
    return ORBFE_OK;
}

extern "C" int orbfe_enqueue_fuse(orbfe_context *ctx, const orbfe_grid_keyframe *kf, const float *Tcw, int n_pts, const int32_t *d_pt_index, int n_rows,
                                  const float *d_pos, const float *d_normal, const float *d_max_distance, const float *d_min_distance,
                                  const uint8_t *d_pt_desc, const int32_t *d_pt_valid, float th, int32_t *d_best_idx, int32_t *d_n_fused,
                                  int32_t *d_status, void *stream)
try {
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    ORBFE_ENTRY(ctx);
    return enqueue_fuse(ctx, 0, kf, Tcw, n_pts, d_pt_index, n_rows, d_pos, d_normal, d_max_distance, d_min_distance, d_pt_desc, d_pt_valid, th, d_best_idx,
                        d_n_fused, d_status, stream);
} ORBFE_CATCH(ctx)

extern "C" int orbfe_enqueue_fuse_sim3(orbfe_context *ctx, const orbfe_grid_keyframe *kf, const float *Scw, int n_pts, const int32_t *d_pt_index, int n_rows,
                                       const float *d_pos, const float *d_normal, const float *d_max_distance, const float *d_min_distance,
                                       const uint8_t *d_pt_desc, const int32_t *d_pt_valid, float th, int32_t *d_best_idx, int32_t *d_n_fused,
                                       int32_t *d_status, void *stream)
try {
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    ORBFE_ENTRY(ctx);
    return enqueue_fuse(ctx, 1, kf, Scw, n_pts, d_pt_index, n_rows, d_pos, d_normal, d_max_distance, d_min_distance, d_pt_desc, d_pt_valid, th, d_best_idx,
                        d_n_fused, d_status, stream);
} ORBFE_CATCH(ctx)
