// orbfe_map_point_device.hip -- the writer of the map-point table: MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:242-307) and
// MapPoint::UpdateNormalAndDepth (:330-371) for chosen rows, from observation lists over device-resident keyframes, asynchronous on the
// caller's stream.  The table (pos, normal, max_distance, min_distance, 32-byte descriptor per row) is what orbfe_enqueue_fuse, the Sim3
// matchers and SearchBySim3's per-slot arrays read; with this call a row recomputed after CreateNewMapPoints, SearchInNeighbors,
// MapPoint::Replace or CorrectLoop never leaves HBM.
//
//   map_point_kernel   one wave per update, four per workgroup, behind a one-thread reset of the status.
//     pass 1   lanes stride over the list: (kf, idx), then the record, both checked before they become addresses; the wave counts the
//              good entries (bad == 0) and learns whether the update is faulty BEFORE anything of its row is written
//     normal   every lane forms the term of its entry (three subtractions, the double norm, alpha, three products), the wave adds the
//              terms in list order by lane read: float addition is not associative, so the order is the reference's
//     descriptor  lane i keeps descriptor i of a block of 64 list entries in eight VGPRs.  G is an order-preserving sub-list, so it needs
//              no physical compaction: the ballot of the good lanes IS G, the columns are its set bits in order, and the first good
//              list position with the smallest median is the first index of G with it.  dist[i][j] is eight xor + popcount against the
//              lane read of descriptor j.  The median needs no sort: it is the smallest v in 0..256 with #{j : dist[i][j] <= v} >= k + 1,
//              nine bisection steps that recompute the distances (no LDS at all: DESIGN.md section 4j).  The winner is the wave minimum
//              of median << 16 | lane.
//              A list of more than 64 entries takes its rows 64 at a time and streams the columns 64 at a time through the same
//              count; blocks are visited in order and compared with <, so the result is the same for any N.
#include "../../include/orbfe.h"
#include "orbfe_config.h"
#include "orbfe_host.h"
#include "orbfe_common.hpp"

static_assert(sizeof(orbfe_obs_keyframe) == 40, "orbfe_obs_keyframe: two pointers, the centre, three ints");

struct MapPointArgs {
    const orbfe_obs_keyframe *kfs;
    const int32_t *row, *obs_off, *obs_kf, *obs_idx, *ref;
    const float *pos;
    float *normal, *max_distance, *min_distance;
    uint8_t *pt_desc;
    int32_t *best, *status;
    int n_kfs, n_upd, n_rows, n_obs, what, nlevels;
    float sf[ORBFE_MAX_LEVELS]; // mvScaleFactors
};

__global__ __launch_bounds__(64) void map_point_reset_kernel(int32_t *status)
{
    if (threadIdx.x == 0) *status = 0;
}

// one observation as a lane holds it; ok: both indices were inside their arrays and the record has descriptors
struct Obs {
    const uint32_t *desc;
    const orbfe_obs_keyframe *kf;
    bool ok, good; // good: ok and the keyframe is not bad
};

// entry o of d_obs_kf / d_obs_idx (o inside [0, n_obs): the caller checked the offsets), every index tested before it is an address
__device__ __forceinline__ Obs load_obs(const MapPointArgs &a, int o, bool active)
{
    Obs e = {nullptr, nullptr, false, false};
    if (!active) return e;
    const int kf = a.obs_kf[o], idx = a.obs_idx[o];
    if (kf < 0 || kf >= a.n_kfs) return e;
    e.kf = a.kfs + kf;
    const uint8_t *d = e.kf->desc;
    if (idx < 0 || idx >= e.kf->n || !d) return e;
    e.desc = (const uint32_t *)(d + (size_t)idx * 32);
    e.ok = true;
    e.good = e.kf->bad == 0;
    return e;
}

__device__ __forceinline__ float lane_read(float v, int j) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j)); }

// how many of the columns `cols` (lanes of cd) are within `v` of the lane's own row descriptor; cols is wave-uniform
__device__ __forceinline__ int count_within(const uint32_t (&rd)[8], const uint32_t (&cd)[8], u64 cols, int v)
{
    int cnt = 0;
    for (; cols; cols &= cols - 1) {
        const int j = __builtin_ctzll(cols);
        int dist = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) dist += __popc(rd[k] ^ (uint32_t)__builtin_amdgcn_readlane((int)cd[k], j));
        cnt += dist <= v;
    }
    return cnt;
}

__global__ __launch_bounds__(256) void map_point_kernel(MapPointArgs a)
{
    const int q = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); // wave-uniform: so is every branch on q, r, n or fault below
    const int lane = threadIdx.x & 63;
    if (q >= a.n_upd) return;
    const int r = a.row ? a.row[q] : q;
    const int o0 = a.obs_off[q], o1 = a.obs_off[q + 1];
    bool fault = r < 0 || r >= a.n_rows || o0 < 0 || o1 < o0 || o1 > a.n_obs;
    const int n = fault ? 0 : o1 - o0;

    // pass 1: the whole list is checked before anything of row r is written
    int n_good = 0;
    for (int base = 0; base < n; base += 64) {
        const bool active = base + lane < n;
        const Obs e = load_obs(a, o0 + base + lane, active);
        if (__ballot(active && !e.ok)) fault = true;
        n_good += __popcll(__ballot(e.good));
    }
    int level = 0;
    float ow_ref[3] = {0.f, 0.f, 0.f};
    if ((a.what & ORBFE_MP_NORMAL_DEPTH) && !fault && n > 0) { // the reference keyframe's entry, read by every lane alike
        const int pr = a.ref[q];
        if (pr < 0 || pr >= n) fault = true;
        else {
            const orbfe_obs_keyframe *kf = a.kfs + a.obs_kf[o0 + pr]; // pass 1 found this entry in range
            const orbfe_keypoint *ku = kf->keys_un;
            if (!ku) fault = true;
            else {
                level = ku[a.obs_idx[o0 + pr]].octave;
                if (level < 0 || level >= a.nlevels) fault = true;
            }
            ow_ref[0] = kf->Ow[0]; ow_ref[1] = kf->Ow[1]; ow_ref[2] = kf->Ow[2];
        }
    }
    if (fault || n == 0) { // MapPoint.cc:256-257, :345-346, or a faulty update: skipped whole
        if (lane == 0) {
            if (fault) *a.status = ORBFE_ERR_INVALID; // every wave that writes writes this value
            if (a.best) a.best[q] = -1;
        }
        return;
    }

    if (a.what & ORBFE_MP_NORMAL_DEPTH) {
        const float P[3] = {a.pos[3 * (size_t)r], a.pos[3 * (size_t)r + 1], a.pos[3 * (size_t)r + 2]};
        float acc[3] = {0.f, 0.f, 0.f};
        for (int base = 0; base < n; base += 64) {
            float t[3] = {0.f, 0.f, 0.f};
            if (base + lane < n) {
                const orbfe_obs_keyframe *kf = a.kfs + a.obs_kf[o0 + base + lane];
                const float d[3] = {__fsub_rn(P[0], kf->Ow[0]), __fsub_rn(P[1], kf->Ow[1]), __fsub_rn(P[2], kf->Ow[2])};
                const double nrm = sqrt((double)d[0] * d[0] + (double)d[1] * d[1] + (double)d[2] * d[2]); // cv::norm
                const float alpha = (float)(1.0 / nrm);                                                   // Mat / double: a scale by 1./s
                t[0] = __fmul_rn(d[0], alpha); t[1] = __fmul_rn(d[1], alpha); t[2] = __fmul_rn(d[2], alpha);
            }
            const int m = n - base < 64 ? n - base : 64;
            for (int j = 0; j < m; j++) { // in list order: normal = normal + normali / norm
                acc[0] = __fadd_rn(lane_read(t[0], j), acc[0]);
                acc[1] = __fadd_rn(lane_read(t[1], j), acc[1]);
                acc[2] = __fadd_rn(lane_read(t[2], j), acc[2]);
            }
        }
        const float inv_n = (float)(1.0 / (double)n); // Mat / int: convertTo with a float scale
        const float d[3] = {__fsub_rn(P[0], ow_ref[0]), __fsub_rn(P[1], ow_ref[1]), __fsub_rn(P[2], ow_ref[2])};
        const float dist = (float)sqrt((double)d[0] * d[0] + (double)d[1] * d[1] + (double)d[2] * d[2]);
        const float max_d = __fmul_rn(dist, a.sf[level]);
        if (lane == 0) {
            a.normal[3 * (size_t)r] = __fmul_rn(acc[0], inv_n);
            a.normal[3 * (size_t)r + 1] = __fmul_rn(acc[1], inv_n);
            a.normal[3 * (size_t)r + 2] = __fmul_rn(acc[2], inv_n);
            a.max_distance[r] = max_d;
            a.min_distance[r] = __fdiv_rn(max_d, a.sf[a.nlevels - 1]);
        }
    }

    int best_pos = -1;
    if ((a.what & ORBFE_MP_DESCRIPTOR) && n_good > 0) {
        const int need = (int)(0.5 * (n_good - 1)) + 1; // the median is the need-th smallest of a row
        int best_median = 257;
        for (int rbase = 0; rbase < n; rbase += 64) {
            const Obs e = load_obs(a, o0 + rbase + lane, rbase + lane < n);
            const u64 rows = __ballot(e.good);
            if (!rows) continue;
            uint32_t rd[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            if (e.good) {
#pragma unroll
                for (int k = 0; k < 8; k++) rd[k] = e.desc[k];
            }
            int lo = 0, hi = 256; // the smallest v with count(v) >= need; count(256) = n_good
            for (int step = 0; step < 9; step++) {
                const int mid = (lo + hi) >> 1;
                int cnt = 0;
                if (n <= 64) cnt = count_within(rd, rd, rows, mid);
                else
                    for (int cbase = 0; cbase < n; cbase += 64) { // the columns, streamed from L2
                        const Obs c = load_obs(a, o0 + cbase + lane, cbase + lane < n);
                        const u64 cols = __ballot(c.good);
                        if (!cols) continue;
                        uint32_t cd[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                        if (c.good) {
#pragma unroll
                            for (int k = 0; k < 8; k++) cd[k] = c.desc[k];
                        }
                        cnt += count_within(rd, cd, cols, mid);
                    }
                if (cnt >= need) hi = mid;
                else lo = mid + 1;
            }
            const unsigned m = wave_min_u32(e.good ? ((unsigned)lo << 16) | (unsigned)lane : ~0u); // the lowest lane wins a tie
            if ((int)(m >> 16) < best_median) { // strict, blocks in order: the first minimum (:296)
                best_median = (int)(m >> 16);
                best_pos = rbase + (int)(m & 0xffffu);
            }
        }
        if (best_pos >= 0) {
            const Obs w = load_obs(a, o0 + best_pos, true);
            if (lane < 8 && w.ok) ((uint32_t *)(a.pt_desc + (size_t)r * 32))[lane] = w.desc[lane];
        }
    }
    if (lane == 0 && a.best) a.best[q] = best_pos;
}

extern "C" int orbfe_enqueue_update_map_points(orbfe_context *ctx, const orbfe_obs_keyframe *d_kfs, int n_kfs, int n_upd, const int32_t *d_row, int n_rows,
                                               const int32_t *d_obs_off, const int32_t *d_obs_kf, const int32_t *d_obs_idx, int n_obs, const int32_t *d_ref,
                                               int what, const float *d_pos, float *d_normal, float *d_max_distance, float *d_min_distance,
                                               uint8_t *d_pt_desc, int32_t *d_best, int32_t *d_status, void *stream)
try {
    ORBFE_ENTRY(ctx);
    // what the arguments alone show is refused first, so that the refusals can be told apart without a device
    if (!d_status) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "update_map_points: null d_status");
    if (n_kfs < 0 || n_upd < 0 || n_rows < 0 || n_obs < 0) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "update_map_points: negative count");
    if (what < 1 || what > (ORBFE_MP_DESCRIPTOR | ORBFE_MP_NORMAL_DEPTH)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "update_map_points: what = %d", what);
    if (!d_row && n_rows < n_upd)
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "update_map_points: %d updates without a row list over a table of %d rows", n_upd, n_rows);
    if (n_upd > 0) {
        if (!d_obs_off || !d_pos) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "update_map_points: null d_obs_off or d_pos");
        if ((what & ORBFE_MP_DESCRIPTOR) && !d_pt_desc) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "update_map_points: null descriptor column");
        if ((what & ORBFE_MP_NORMAL_DEPTH) && (!d_normal || !d_max_distance || !d_min_distance))
            return orbfe_fail(ctx, ORBFE_ERR_INVALID, "update_map_points: null normal or distance column");
        if ((what & ORBFE_MP_NORMAL_DEPTH) && !d_ref) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "update_map_points: null d_ref");
        if (n_obs > 0 && (!d_kfs || !d_obs_kf || !d_obs_idx))
            return orbfe_fail(ctx, ORBFE_ERR_INVALID, "update_map_points: null keyframe directory or observation list");
    }
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    MapPointArgs a;
    a.nlevels = ctx->params.nlevels;
    if (a.nlevels < 1 || a.nlevels > ORBFE_MAX_LEVELS) return orbfe_fail(ctx, ORBFE_ERR_UNSUPPORTED, "nlevels = %d", a.nlevels);
    const float *sf = ctx->plan.scale;
    for (int l = 0; l < ORBFE_MAX_LEVELS; l++) a.sf[l] = l < a.nlevels ? sf[l] : 1.f;
    a.kfs = d_kfs; a.row = d_row; a.obs_off = d_obs_off; a.obs_kf = d_obs_kf; a.obs_idx = d_obs_idx; a.ref = d_ref;
    a.pos = d_pos; a.normal = d_normal; a.max_distance = d_max_distance; a.min_distance = d_min_distance; a.pt_desc = d_pt_desc;
    a.best = d_best; a.status = d_status;
    a.n_kfs = n_kfs; a.n_upd = n_upd; a.n_rows = n_rows; a.n_obs = n_obs; a.what = what;
    hipStream_t s;
    if (const int rc = orbfe_enqueue_on(ctx, stream, false, &s)) return rc;
    hipLaunchKernelGGL(map_point_reset_kernel, dim3(1), dim3(64), 0, s, d_status);
    if (n_upd > 0) hipLaunchKernelGGL(map_point_kernel, dim3((n_upd + 3) / 4), dim3(256), 0, s, a);
    ORBFE_HIP_TRY(ctx, hipGetLastError());
    return ORBFE_OK;
} ORBFE_CATCH(ctx)
