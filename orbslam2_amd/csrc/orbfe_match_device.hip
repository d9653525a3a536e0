// orbfe_match_device.hip -- the two per-frame matchers of Tracking on device-resident data, asynchronous on the caller's stream:
// SearchByProjection(CurrentFrame, LastFrame, th, bMono) (src/ORBmatcher.cc:1324-1466), Frame::isInFrustum (src/Frame.cc:256-315)
// and SearchByProjection(F, vpMapPoints, th) (src/ORBmatcher.cc:43-135).  Device pointers in, matches in HBM, no host wait.
//
// orbfe_match.hip is the synchronous form and the second implementation this one is tested against: there the map points are
// projected on the host, the four best keys per query come back over the link and orbfe_match_resolve.h replays the accept
// rules.  Here the same steps are kernels:
//   grid_build_kernel     Frame::AssignFeaturesToGrid in one workgroup, for this path (the slot's keypoint count read from the
//                         extraction's counter) and, through orbfe_launch_grid_build, for orbfe_match.hip
//   window_topk_kernel    one wave per map point: its 32-byte MatchQuery (the per-point functions of orbfe_match_resolve.h), then
//                         GetFeaturesInArea + Hamming distances, the 4 smallest statically admissible keys
//   frustum_kernel        Frame::isInFrustum, one lane per map point
//   resolve_kernel        ONE workgroup replays the sequentially greedy accept rules in query order (see there)
//   gather_kernel         optional has_point / Xw for orbfe_enqueue_pose_optimization
// and SearchByProjection(CurrentFrame, KeyFrame, sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:1468-1595) for every candidate of a
// relocalisation (src/Tracking.cc:1540-1580) through the same kernels: a grid row (window, gather) or a workgroup (resolve) per
// candidate, whose arguments come from its orbfe_reloc_candidate record (KfBatch); kf_prepare_kernel builds sAlreadyFound and the
// keypoints' has-point flags from cur_point first.
// SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) of LoopClosing::ComputeSim3 (src/ORBmatcher.cc:285-398) runs through the window
// and resolve kernels as well, against an orbfe_grid_keyframe record instead of an image slot (Sim3Source; Sim3Points, the PointTable of
// orbfe_match_window.hpp that orbfe_fuse_device.hip reads too): the keyframe rule with the keypoints matched on entry as static blocks
// and TH_LOW as the bound.  Its grid and keypoints are the caller's uploads,
// so it has instantiations of its own (CHECKED) in which both walks -- the top-4 pass and wave 0's rescan -- test offsets, indices and
// octaves before they become addresses; the instantiations of the matchers above are what they were.
// Every source projects against a View (orbfe_match_resolve.h: camera, scale factors, bounds), built on the host by orbfe_view.
// The grid cell, the window, its walk, the candidate key and the top-4 selection are orbfe_match_window.hpp, shared with
// orbfe_match.hip; the smallest key is the reference loop's first minimum.  No candidate list is kept: a query whose four keys are
// all taken recomputes its window.
#include "../../include/orbfe.h"
#include "orbfe_device.h"
#include "orbfe_host.h"
#include "orbfe_match_resolve.h"
#include "orbfe_match_window.hpp"

#include <algorithm>
#include <new>
#include <vector>

#define TOPK 4
#define RESOLVE_THREADS 512 // queries evaluated per step of the resolve kernel
#define RESOLVE_CHUNK 1024  // queries staged in LDS at a time
#define Q_BAD 4 // MatchQuery::flags bit of the device path: the point's octave / predicted level is out of range

using orbfe_resolve::HISTO_LENGTH;
using orbfe_resolve::key_dist;
using orbfe_resolve::key_idx;
using orbfe_resolve::key_level;
using orbfe_resolve::MatchQuery;
using orbfe_resolve::TH_HIGH;
using orbfe_resolve::TH_LOW;
using orbfe_resolve::View;

// Frame::AssignFeaturesToGrid in one workgroup: count, scan and fill over LDS counters
__global__ __launch_bounds__(1024) void grid_build_kernel(GridFrame f)
{
    __shared__ int s_cnt[GRID_CELLS];
    __shared__ int s_scan[1024];
    const int tid = threadIdx.x, n = frame_count(f);
    for (int c = tid; c < GRID_CELLS; c += 1024) s_cnt[c] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 1024) {
        const int c = grid_cell(f, i);
        if (c >= 0) atomicAdd(&s_cnt[c], 1);
    }
    __syncthreads();
    const int per = GRID_CELLS / 1024; // 3
    int sum = 0;
    for (int k = 0; k < per; k++) sum += s_cnt[tid * per + k];
    s_scan[tid] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int v = tid >= o ? s_scan[tid - o] : 0;
        __syncthreads();
        s_scan[tid] += v;
        __syncthreads();
    }
    int run = s_scan[tid] - sum;
    for (int k = 0; k < per; k++) {
        const int c = tid * per + k, v = s_cnt[c];
        f.cell_off[c] = run;
        s_cnt[c] = run; // becomes the fill cursor
        run += v;
    }
    if (tid == 1023) f.cell_off[GRID_CELLS] = s_scan[1023];
    __syncthreads();
    for (int i = tid; i < n; i += 1024) {
        const int c = grid_cell(f, i);
        if (c >= 0) f.cell_idx[atomicAdd(&s_cnt[c], 1)] = i; // order inside a cell is irrelevant (keys carry it)
    }
}
static_assert(GRID_CELLS % 1024 == 0, "grid_build_kernel gives every thread the same number of cells");

// What the window kernel reads and writes for one row of its grid (blockIdx.y): the launch's arguments, which a source with more
// than one row (KfBatch) replaces by that row's
struct WindowRow {
    MatchQuery *q;
    const uint8_t *qdesc;
    int nq;
    const uint8_t *blocked0;
    unsigned long long *topk;
    int *n_static;
    int32_t *cur_match;
};

// ---- projection: where a query comes from.  The window kernel asks for query i (every lane of its wave states the same
// arithmetic), so the matchers need no launch of their own for it ----
struct LastSource { // SearchByProjection(CurrentFrame, LastFrame, th, bMono)
    View V;
    const float *Tcw_cur, *Tcw_last, *pos;
    const int32_t *valid, *octave;
    float th;
    int mono;
    __device__ __forceinline__ const LastSource &row(int, WindowRow &) const { return *this; }
    __device__ __forceinline__ MatchQuery query(int i) const
    {
        float Tc[12], Tl[12];
        for (int k = 0; k < 12; k++) { Tc[k] = Tcw_cur[k]; Tl[k] = Tcw_last[k]; }
        bool forward, backward;
        orbfe_resolve::last_motion(V.C, Tc, Tl, mono, forward, backward);
        MatchQuery Q = {0, 0, 0, 0, -1, 0, 0, 0};
        const float p[3] = {pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]};
        if (orbfe_resolve::query_last_point(V, Tc, forward, backward, p, valid[i], octave[i], th, Q) < 0) Q.flags = Q_BAD;
        return Q;
    }
};
struct PointsSource { // SearchByProjection(F, vpMapPoints, th)
    View V;
    const orbfe_track_point *pts;
    float th;
    __device__ __forceinline__ const PointsSource &row(int, WindowRow &) const { return *this; }
    __device__ __forceinline__ MatchQuery query(int i) const
    {
        MatchQuery Q = {0, 0, 0, 0, -1, 0, 0, 0};
        const orbfe_track_point pt = pts[i];
        if (orbfe_resolve::query_track_point(V.sf, V.nlevels, pt, th, Q) < 0) Q.flags = Q_BAD;
        return Q;
    }
};

struct ResolveArgs;
// SearchByProjection(pKF, Scw, vpPoints, vpMatched, th): the point table (orbfe_match_window.hpp) as both kernels of the matcher need it
struct Sim3Points : PointTable {
    int nlevels;
    int32_t *pt_match; // [n_pts] the keypoint query q took, or -1
    __device__ __forceinline__ void resolve(int, ResolveArgs &) const {}
};
struct Sim3Source {
    View V; // with the keyframe's bounds
    Sim3Points pts;
    int kf_n;
    float T[12], ow[3]; // [R|t] of the decomposed Scw and the camera centre, both computed on the host
    float th;
    __device__ __forceinline__ const Sim3Source &row(int, WindowRow &) const { return *this; }
    __device__ __forceinline__ const uint8_t *desc(int q) const { return pts.desc(q); }
    __device__ __forceinline__ int nlevels() const { return V.nlevels; }
    __device__ __forceinline__ MatchQuery query(int q) const
    {
        MatchQuery Q = {0, 0, 0, 0, -1, 0, 0, 0};
        if (kf_n == 0) return Q; // a keyframe without keypoints has no window: neither its arrays nor the table's are read
        const int row = pts.row(q);
        if (row < 0) { Q.flags = Q_BAD; return Q; }
        float ur; // not used by this matcher
        const float p[3] = {pts.pos[3 * (size_t)row], pts.pos[3 * (size_t)row + 1], pts.pos[3 * (size_t)row + 2]};
        const float nr[3] = {pts.normal[3 * (size_t)row], pts.normal[3 * (size_t)row + 1], pts.normal[3 * (size_t)row + 2]};
        // exactly as sim3_projection_impl mode 0 (orbfe_match.hip) calls it
        orbfe_resolve::query_fuse_point(V, T, ow, 0, p, nr, pts.pt_valid[q], pts.max_distance[row], pts.min_distance[row], th, Q, &ur);
        return Q;
    }
};

__global__ __launch_bounds__(256) void frustum_kernel(View V, const float *__restrict__ Tcw, int n, const float *__restrict__ pos,
                                                      const float *__restrict__ normal, const float *__restrict__ max_distance,
                                                      const float *__restrict__ min_distance, float viewing_cos_limit, orbfe_track_point *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float T[12], ow[3];
    for (int k = 0; k < 12; k++) T[k] = Tcw[k];
    orbfe_resolve::camera_center(T, ow);
    const float p[3] = {pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]}, nr[3] = {normal[3 * i], normal[3 * i + 1], normal[3 * i + 2]};
    orbfe_track_point o;
    orbfe_resolve::frustum_point(V, T, ow, p, nr, max_distance[i], min_distance[i], viewing_cos_limit, o);
    out[i] = o;
}

// ---- window query ----
// One wave per query: the map point is projected into its MatchQuery (kept in q[] for the resolve kernel's re-scans), then every
// lane keeps the TOPK smallest admissible keys of its own cells in registers and the wave merges them: any window size, no staging.
// n_static = how many keys passed the static filters, -1 for a Q_BAD query.  The threads below the frame's keypoint count also
// reset cur_match (the launch covers the keypoint capacity).
// CHECKED (a keyframe record): the query's descriptor is the source's to find, the walk is the checked one and a walk that failed
// makes the query a Q_BAD one, which the resolve kernel reports.
template <class Source, bool CHECKED = false>
__global__ __launch_bounds__(256) void window_topk_kernel(GridFrame f, Source src0, WindowRow r)
{
    const auto &src = src0.row(blockIdx.y, r); // the source and the arguments of this row
    const int gid = blockIdx.x * 256 + threadIdx.x;
    if (gid < frame_count(f)) r.cur_match[gid] = -1;
    const int iq = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (iq >= r.nq) return;
    const MatchQuery Q = src.query(iq);
    if (lane == 0) r.q[iq] = Q;
    const Window w = query_window(f, Q);
    Top4 top;
    int passed = 0;
    bool ok = true;
    const auto emit = [&](unsigned long long key, int idx) {
        if (key_dist(key) >= 256 || (r.blocked0 && r.blocked0[idx])) return; // static filters
        passed++;
        top.insert(key);
    };
    if (w.ncells > 0) {
        if constexpr (CHECKED) ok = scan_window<true>(f, Q, w, (const uint32_t *)src.desc(iq), lane, emit, f.cap, src.nlevels());
        else scan_window(f, Q, w, (const uint32_t *)(r.qdesc + (size_t)iq * 32), lane, emit);
    }
    if constexpr (CHECKED) ok = __all(ok) != 0;
    passed = wave_sum_i32(passed);
    for (int k = 0; k < TOPK; k++) {
        const unsigned long long m = top.pop_wave_min();
        if (lane == 0) r.topk[(size_t)iq * TOPK + k] = m;
    }
    if (lane == 0) r.n_static[iq] = ((Q.flags & Q_BAD) || !ok) ? -1 : passed;
}

// ---- resolve ----
struct GatherRow { // what gather_kernel reads and writes for one row
    const int32_t *cur_match;
    const float *pos;
    int32_t *cur_point; // null but for the keyframe matcher
    uint8_t *has_point;
    float *Xw;
};
struct ResolveArgs {
    GridFrame f;
    const MatchQuery *q;
    const uint8_t *qdesc;
    int nq;
    const unsigned long long *topk;
    const int *n_static;
    const int32_t *obs;       // Observations() of the map point of query i; null: every accepted keypoint is closed (the keyframe rule)
    const float *angle;       // last_angle (check_ori), else null
    const uint8_t *blocked0;  // keypoints taken before the call, or null
    int points;               // 0: the last-frame rule, 1: the local-map rule (best / second best, nnratio)
    int th_high;              // the largest accepted distance: TH_HIGH, or ORBdist of the keyframe rule
    int check_ori;
    float nnratio;
    int row_err;              // the row's arguments were refused before the kernel looked at a query
    int32_t *ev;              // [nq] scratch: keypoint accepted by query i, or -1
    int32_t *cur_match, *nmatches, *status;
};

__device__ __forceinline__ bool blk_test(const uint32_t *blk, int idx) { return (blk[idx >> 5] >> (idx & 31)) & 1u; }

// What the resolve kernel keeps of a candidate key: dist << 24 | octave << 16 | idx.  The order of a query's keys is their position
// in its prefix, so 32 bits are enough; admissible keys have dist < 256 and idx < 65535, so NO_PKEY is no key.
#define NO_PKEY 0xffffffffu
__device__ __forceinline__ uint32_t pack_key(unsigned long long k)
{
    return k == NO_KEY ? NO_PKEY : ((uint32_t)key_dist(k) << 24) | ((uint32_t)key_level(k) << 16) | (uint32_t)key_idx(k);
}
__device__ __forceinline__ int pkey_idx(uint32_t k) { return (int)(k & 0xffffu); }
// the accept rules of resolve_last / resolve_kf / resolve_points (orbfe_match_resolve.h) for one query, given its best and second-best free key
__device__ __forceinline__ bool accept_rule(int points, int th_high, float nnratio, uint32_t best, uint32_t second)
{
    if (best == NO_PKEY) return false;
    const int best_dist = (int)(best >> 24);
    if (!points) return best_dist <= th_high;
    const int best_level = (int)((best >> 16) & 255u);
    const int best_dist2 = second != NO_PKEY ? (int)(second >> 24) : 256, best_level2 = second != NO_PKEY ? (int)((second >> 16) & 255u) : -1;
    if (best_dist > th_high) return false;
    return !(best_level == best_level2 && (float)best_dist > nnratio * (float)best_dist2);
}

// One workgroup per row of the call (one row, or one per relocalisation candidate: rows.resolve replaces the arguments by those of
// row blockIdx.x).  The accept rules are sequential only through the `blocked` flags (a keypoint taken by a map point with
// observations -- under the keyframe rule, by any map point -- is closed to every later query), and the flags only ever go from
// free to blocked.  So the workgroup
// evaluates RESOLVE_THREADS consecutive queries at once against the current flags (512: measured best of 256 / 512 / 1024 -- a step
// costs about a microsecond at any of these widths, a narrower one needs more steps, a wider one dearer barriers); a thread's answer is final unless an
// EARLIER thread of the same step blocks a keypoint that this thread looked at and found free (its best, for the local-map
// rule also its second best).  Every thread that would block a keypoint posts its index into a claim table (LDS, atomic
// minimum, hashed by keypoint: a collision can only report a conflict that is none, which costs a step, never an answer);
// the threads before the first conflict -- or before the first query whose four-key prefix ran out -- commit, the window
// slides there and the rest are evaluated again.  At least one query commits per step, so the loop ends after at most nq steps.
// A query whose prefix ran out (all of its keys blocked, more than TOPK statically admissible ones) gets its window scanned
// again by wave 0 for the smallest keys that pass the static filters AND the current flags: exact, never a truncated answer.
// cur_match[k] = the LAST query that took keypoint k = the largest index: an atomic maximum, so no store order matters.
// LDS: blocked bitmask 8 KB (65536 keypoints) + claim table 16 KB + RESOLVE_CHUNK x (4 packed keys 16 B + event 4 B + n_static
// and observation flag 2 B) = 46 KB.
#define CLAIM_SLOTS 4096
#define NO_CLAIM 0x7fffffff
struct OneRow { // the three matchers of one row: the launch's arguments are the row's
    __device__ __forceinline__ void resolve(int, ResolveArgs &) const {}
    __device__ __forceinline__ void gather(int, GatherRow &) const {}
};
// CHECKED (Rows = Sim3Points, a keyframe record): wave 0's rescan is the checked walk, a query's descriptor is the table row its index
// names, and every query's event is also stored per query (rows.pt_match).
template <class Rows, bool CHECKED = false>
__global__ __launch_bounds__(RESOLVE_THREADS) void resolve_kernel(ResolveArgs a, Rows rows)
{
    rows.resolve(blockIdx.x, a);
    __shared__ uint32_t s_blk[65536 / 32];
    __shared__ int s_claim[CLAIM_SLOTS];
    __shared__ uint32_t s_keys[TOPK][RESOLVE_CHUNK]; // packed key k of every query side by side: conflict-free reads
    __shared__ int s_ev[RESOLVE_CHUNK];   // keypoint accepted by the chunk's query, or -1
    __shared__ int8_t s_ns[RESOLVE_CHUNK]; // n_static clamped to [-1, TOPK + 1]
    __shared__ uint8_t s_obs[RESOLVE_CHUNK];
    __shared__ int s_hist[32];
    __shared__ int s_nm, s_err, s_keep[3], s_stop;
    const int tid = threadIdx.x, lane = tid & 63;
    const int n = frame_count(a.f);
    for (int w = tid; w < 65536 / 32; w += RESOLVE_THREADS) s_blk[w] = 0;
    for (int w = tid; w < CLAIM_SLOTS; w += RESOLVE_THREADS) s_claim[w] = NO_CLAIM;
    if (tid < 32) s_hist[tid] = 0;
    if (tid == 0) { s_nm = 0; s_err = a.row_err; }
    __syncthreads();
    if (a.blocked0)
        for (int k = tid; k < n; k += RESOLVE_THREADS)
            if (a.blocked0[k]) atomicOr(&s_blk[k >> 5], 1u << (k & 31));
    for (int base = 0; base < a.nq; base += RESOLVE_CHUNK) {
        const int cnt = a.nq - base < RESOLVE_CHUNK ? a.nq - base : RESOLVE_CHUNK;
        for (int t = tid; t < cnt; t += RESOLVE_THREADS) { // stage the chunk
            const ulonglong2 *tk = (const ulonglong2 *)(a.topk + (size_t)(base + t) * TOPK);
            const ulonglong2 k01 = tk[0], k23 = tk[1];
            s_keys[0][t] = pack_key(k01.x); s_keys[1][t] = pack_key(k01.y); s_keys[2][t] = pack_key(k23.x); s_keys[3][t] = pack_key(k23.y);
            const int ns = a.n_static[base + t];
            s_ns[t] = (int8_t)(ns < 0 ? -1 : (ns > TOPK ? TOPK + 1 : ns));
            s_obs[t] = a.obs ? a.obs[base + t] > 0 : 1;
            if (ns < 0) s_err = 1;
        }
        __syncthreads(); // also: the flags of blocked0 are set, the previous chunk's events are consumed
        int b = 0;       // the same in every thread
        while (b < cnt) {
            const int j = b + tid;
            const bool active = j < cnt;
            uint32_t best = NO_PKEY, second = NO_PKEY;
            bool need_full = false;
            if (active) {
                // the four keys and their flags are read at once (two LDS round trips instead of eight dependent ones); the keys
                // ascend and NO_PKEY pads the end, whose index 0xffff reads a valid flag word
                uint32_t key[TOPK];
                bool free_[TOPK];
#pragma unroll
                for (int k = 0; k < TOPK; k++) key[k] = s_keys[k][j];
#pragma unroll
                for (int k = 0; k < TOPK; k++) free_[k] = !blk_test(s_blk, pkey_idx(key[k])) && key[k] != NO_PKEY;
#pragma unroll
                for (int k = TOPK - 1; k >= 0; k--)
                    if (free_[k]) { second = best; best = key[k]; } // ends with the first free key in best, the next free one in second
                if (!a.points) second = NO_PKEY;
                const bool found = a.points ? second != NO_PKEY : best != NO_PKEY;
                need_full = !found && s_ns[j] > TOPK; // the prefix ran out before the answer was found
            }
            const bool acc = active && !need_full && accept_rule(a.points, a.th_high, a.nnratio, best, second);
            const int e1 = best != NO_PKEY ? pkey_idx(best) : -1, e2 = second != NO_PKEY ? pkey_idx(second) : -1;
            const int blocks = (acc && s_obs[active ? j : 0]) ? e1 : -1; // the keypoint this thread closes
            if (tid == 0) s_stop = NO_CLAIM;
            if (blocks >= 0) atomicMin(&s_claim[blocks & (CLAIM_SLOTS - 1)], tid);
            __syncthreads();
            const bool conflict = (e1 >= 0 && s_claim[e1 & (CLAIM_SLOTS - 1)] < tid) || (e2 >= 0 && s_claim[e2 & (CLAIM_SLOTS - 1)] < tid);
            if (active && (conflict || need_full)) atomicMin(&s_stop, 2 * tid + (need_full ? 0 : 1)); // need_full stays true whatever commits before
            __syncthreads();
            const int stop = s_stop;
            const int left = cnt - b < RESOLVE_THREADS ? cnt - b : RESOLVE_THREADS;
            const int fstop = stop == NO_CLAIM ? left : stop >> 1;       // threads below commit
            const bool full = stop != NO_CLAIM && !(stop & 1);           // query b + fstop needs its window scanned again
            if (blocks >= 0) s_claim[blocks & (CLAIM_SLOTS - 1)] = NO_CLAIM; // every claimant clears its slot
            const bool commit = tid < fstop;
            if (commit) {
                s_ev[j] = acc ? e1 : -1;
                if (blocks >= 0) atomicOr(&s_blk[blocks >> 5], 1u << (blocks & 31));
            }
            const int wave_acc = __popcll(__ballot(commit && acc));
            if (lane == 0 && wave_acc) atomicAdd(&s_nm, wave_acc);
            __syncthreads(); // the flags, the claim table and s_stop are settled for the next step
            b += fstop;
            if (!full) continue;
            if (tid < 64) { // wave 0 scans the window of query b again under the current flags
                const int gq = base + b;
                const MatchQuery Q = a.q[gq];
                const Window w = query_window(a.f, Q);
                unsigned long long t0 = NO_KEY, t1 = NO_KEY;
                const auto emit = [&](unsigned long long key, int idx) {
                    if (key_dist(key) >= 256 || blk_test(s_blk, idx)) return; // s_blk holds the static blocks too
                    if (key < t1) {
                        t1 = key;
                        if (t1 < t0) { const unsigned long long x = t0; t0 = t1; t1 = x; }
                    }
                };
                if (w.ncells > 0) {
                    if constexpr (CHECKED) {
                        const bool ok = scan_window<true>(a.f, Q, w, (const uint32_t *)rows.desc(gq), lane, emit, n, rows.nlevels);
                        if (!__all(ok) && lane == 0) s_err = 1;
                    } else scan_window(a.f, Q, w, (const uint32_t *)(a.qdesc + (size_t)gq * 32), lane, emit);
                }
                const unsigned long long fbest = wave_min_u64(t0);
                const unsigned long long fsecond = wave_min_u64((fbest != NO_KEY && t0 == fbest) ? t1 : t0);
                const bool facc = accept_rule(a.points, a.th_high, a.nnratio, pack_key(fbest), pack_key(fsecond));
                if (lane == 0) {
                    s_ev[b] = facc ? key_idx(fbest) : -1;
                    if (facc) s_nm += 1; // no other thread touches s_nm between the two barriers around this block
                    if (facc && s_obs[b]) atomicOr(&s_blk[key_idx(fbest) >> 5], 1u << (key_idx(fbest) & 31));
                }
            }
            __syncthreads();
            b += 1;
        }
        // the chunk's events: the last query that took a keypoint keeps it; rotHist[bin].push_back(bestIdx2), src/ORBmatcher.cc:1436-1445
        for (int t = tid; t < cnt; t += RESOLVE_THREADS) {
            const int kp = s_ev[t];
            if (kp >= 0) atomicMax(&a.cur_match[kp], base + t);
            if constexpr (CHECKED) rows.pt_match[base + t] = kp;
            if (a.check_ori) {
                int e = -1;
                if (kp >= 0) {
                    const int bin = orbfe_resolve::rot_bin(a.angle[base + t], a.f.keys[kp].angle);
                    atomicAdd(&s_hist[bin], 1);
                    e = kp | (bin << 16);
                }
                a.ev[base + t] = e; // read back by this very thread below
            }
        }
    }
    if (a.check_ori) {
        __syncthreads();
        if (tid < 64) { // ComputeThreeMaxima as three_maxima (orbfe_match_resolve.h) states it, one bin per lane
            const int sz = lane < HISTO_LENGTH ? s_hist[lane] : 0;
            unsigned long long key = sz > 0 ? ((unsigned long long)sz << 32) | (unsigned)(0x7fffffff - lane) : 0ull; // 0: empty bin
            int ind[3] = {-1, -1, -1}, val[3] = {0, 0, 0};
            for (int r = 0; r < 3; r++) {
                const unsigned long long m = ~wave_min_u64(~key); // the largest remaining (size, -index)
                if (m == 0ull) break;
                ind[r] = 0x7fffffff - (int)(unsigned)m;
                val[r] = (int)(m >> 32);
                if (key == m) key = 0ull;
            }
            if ((float)val[1] < 0.1f * (float)val[0]) { ind[1] = -1; ind[2] = -1; } // :1628-1637
            else if ((float)val[2] < 0.1f * (float)val[0]) ind[2] = -1;
            if (lane == 0) { s_keep[0] = ind[0]; s_keep[1] = ind[1]; s_keep[2] = ind[2]; }
        }
        __syncthreads(); // also orders the atomic maxima above before the stores below
        for (int i = tid; i < a.nq; i += RESOLVE_THREADS) {
            const int e = a.ev[i];
            if (e < 0) continue;
            const int bin = e >> 16;
            if (bin != s_keep[0] && bin != s_keep[1] && bin != s_keep[2]) { // once per event, duplicates included (:1452-1463)
                a.cur_match[e & 0xffff] = -1;
                atomicSub(&s_nm, 1);
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        *a.nmatches = s_nm;
        *a.status = s_err ? ORBFE_ERR_INVALID : ORBFE_OK;
    }
}
static_assert(RESOLVE_CHUNK % RESOLVE_THREADS == 0, "resolve_kernel: the thread that stores an event of a chunk reads it back in the last pass");

// mvpMapPoints of the matched keypoints as orbfe_enqueue_pose_optimization reads them, one grid row per row of the call.  With
// cur_point (the keyframe matcher: the map point every keypoint holds, in/out) a new match is entered there and the outputs
// cover the points held before the call too.
template <class Rows>
__global__ __launch_bounds__(256) void gather_kernel(GridFrame f, GatherRow g, Rows rows)
{
    rows.gather(blockIdx.y, g);
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= frame_count(f)) return;
    int m = g.cur_match[k];
    if (g.cur_point) {
        if (m >= 0) g.cur_point[k] = m;
        else m = g.cur_point[k]; // in [-1, n): kf_prepare_kernel checked it
    }
    if (g.has_point) g.has_point[k] = m >= 0;
    if (g.Xw && g.pos && m >= 0) {
        g.Xw[3 * k] = g.pos[3 * m];
        g.Xw[3 * k + 1] = g.pos[3 * m + 1];
        g.Xw[3 * k + 2] = g.pos[3 * m + 2];
    }
}

// ---- SearchByProjection(CurrentFrame, KeyFrame, sAlreadyFound, th, ORBdist) for the candidates of a relocalisation ----
// The candidates of one call: a device array of records, or (cands == null) the single call's record by value.  Row c of every
// scratch array belongs to candidate c: found / q / topk / n_static / ev [n_cands][max_n], held [n_cands][cap], err [n_cands].
struct KfRowSource { // one candidate as the window kernel's source
    const View &V;
    orbfe_reloc_candidate rec;
    const uint8_t *found;
    __device__ __forceinline__ MatchQuery query(int i) const
    {
        float Tc[12], ow[3];
        for (int k = 0; k < 12; k++) Tc[k] = rec.Tcw[k];
        orbfe_resolve::camera_center(Tc, ow);
        MatchQuery Q = {0, 0, 0, 0, -1, 0, 0, 0};
        const float p[3] = {rec.pos[3 * i], rec.pos[3 * i + 1], rec.pos[3 * i + 2]};
        orbfe_resolve::query_kf_point(V, Tc, ow, p, rec.valid[i] && !found[i], rec.max_distance[i], rec.min_distance[i], rec.th, Q);
        return Q;
    }
};
struct KfBatch {
    View V;
    const orbfe_reloc_candidate *cands;
    orbfe_reloc_candidate one;
    int max_n, cap, exclude_held;
    uint8_t *found, *held;
    int32_t *err;
    MatchQuery *q; // the scratch rows of the window and resolve kernels
    unsigned long long *topk;
    int *n_static;
    int32_t *ev;
    int32_t *cur_match, *nmatches, *status; // the outputs, a row per candidate
    uint8_t *has_point;
    float *Xw;

    // Record c with its counts checked BEFORE any of its pointers is followed: a refused record comes back as a keyframe without
    // points whose cur_point and outlier are not read either.
    __device__ __forceinline__ orbfe_reloc_candidate record(int c, bool &refused) const
    {
        orbfe_reloc_candidate r = cands ? cands[c] : one;
        refused = r.n < 0 || r.n > max_n ||
                  (r.n > 0 && (!r.Tcw || !r.pos || !r.desc || !r.valid || !r.angle || !r.max_distance || !r.min_distance || !r.cur_point));
        if (refused) { r.n = 0; r.cur_point = nullptr; r.outlier = nullptr; }
        return r;
    }
    __device__ __forceinline__ KfRowSource row(int c, WindowRow &w) const
    {
        bool refused;
        const KfRowSource s = {V, record(c, refused), found + (size_t)c * max_n};
        w.q = q + (size_t)c * max_n; w.topk = topk + (size_t)c * max_n * TOPK; w.n_static = n_static + (size_t)c * max_n;
        w.qdesc = s.rec.desc; w.nq = s.rec.n;
        w.blocked0 = held + (size_t)c * cap;
        w.cur_match = cur_match + (size_t)c * cap;
        return s;
    }
    __device__ __forceinline__ void resolve(int c, ResolveArgs &a) const
    {
        bool refused;
        const orbfe_reloc_candidate r = record(c, refused);
        a.q = q + (size_t)c * max_n; a.topk = topk + (size_t)c * max_n * TOPK; a.n_static = n_static + (size_t)c * max_n; a.ev = ev + (size_t)c * max_n;
        a.qdesc = r.desc; a.nq = r.n; a.angle = r.angle; a.th_high = r.orb_dist;
        a.blocked0 = held + (size_t)c * cap;
        a.row_err = refused || err[c];
        a.cur_match = cur_match + (size_t)c * cap; a.nmatches = nmatches + c; a.status = status + c;
    }
    __device__ __forceinline__ void gather(int c, GatherRow &g) const
    {
        bool refused;
        const orbfe_reloc_candidate r = record(c, refused);
        g.cur_match = cur_match + (size_t)c * cap; g.pos = r.pos; g.cur_point = r.cur_point;
        g.has_point = has_point ? has_point + (size_t)c * cap : nullptr;
        g.Xw = Xw ? Xw + (size_t)c * cap * 3 : nullptr;
    }
};

// One workgroup per candidate, before its window queries: found[i] = some keypoint holds map point i at entry (sAlreadyFound of
// src/Tracking.cc:1552,1566; only with exclude_held), then the outlier clear of :1545-1547 on cur_point, and held[k] = keypoint k
// still holds a point, the has-point flags the matcher starts from.  A cur_point outside [-1, n) is reported in err and becomes
// -1 before anything uses it as an index.
__global__ __launch_bounds__(1024) void kf_prepare_kernel(GridFrame f, KfBatch b)
{
    __shared__ int s_err;
    const int c = blockIdx.x, tid = threadIdx.x, count = frame_count(f);
    bool refused;
    const orbfe_reloc_candidate r = b.record(c, refused);
    uint8_t *found = b.found + (size_t)c * b.max_n, *held = b.held + (size_t)c * b.cap;
    if (tid == 0) s_err = 0;
    for (int i = tid; i < r.n; i += 1024) found[i] = 0;
    __syncthreads(); // the flags are cleared (the workgroup's own global stores) before any is set
    for (int k = tid; k < count; k += 1024) {
        int p = r.cur_point ? r.cur_point[k] : -1;
        if (p < -1 || p >= r.n) { s_err = 1; p = -1; }
        if (p >= 0 && b.exclude_held) found[p] = 1;
        if (r.outlier && r.outlier[k]) p = -1;
        if (r.cur_point) r.cur_point[k] = p;
        held[k] = p >= 0;
    }
    __syncthreads();
    if (tid == 0) b.err[c] = s_err;
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
struct orbfe_match_device_state {
    DevBuf q, topk, n_static, ev, cells, keys_un, found, held, err, sim3; // grow-only scratch; calls of one context share it, so they are queued in stream order
    std::vector<unsigned> un_epoch;               // per image slot: the extraction call whose keypoints keys_un holds undistorted
    int un_ndist = 0;                             // ... with these coefficients (orbfe_set_distortion may change them between calls)
    float un_dist[5] = {0, 0, 0, 0, 0};
    unsigned grid_epoch = 0;                      // the grid in `cells`: slot grid_slot of extraction call grid_epoch, these keys and bounds
    int grid_slot = -1;
    const void *grid_keys = nullptr;
    float grid_bounds[4] = {0, 0, 0, 0};
};
void orbfe_match_device_state_destroy(orbfe_match_device_state *s) { delete s; }
void orbfe_launch_grid_build(const GridFrame &f, hipStream_t s) { hipLaunchKernelGGL(grid_build_kernel, dim3(1), dim3(1024), 0, s, f); }
orbfe_match_device_state *orbfe_ctx_match_device_state(orbfe_context *ctx)
{
    if (!ctx->match_device) ctx->match_device = new (std::nothrow) orbfe_match_device_state();
    return ctx->match_device;
}

// the two one-way results of orbfe_enqueue_search_by_sim3 (orbfe_sim3_device.hip): n int32_t of the context's grow-only scratch
int32_t *orbfe_ctx_sim3_scratch(orbfe_context *ctx, size_t n)
{
    orbfe_match_device_state *st = orbfe_ctx_match_device_state(ctx);
    if (!st || st->sim3.ensure(sizeof(int32_t) * (n > 0 ? n : 1))) return nullptr;
    return (int32_t *)st->sim3.p;
}


// a Frame's view: its bounds are the floats they are given as
static View frame_view(orbfe_context *ctx, const float *bounds) { return orbfe_view(ctx, bounds[0], bounds[1], bounds[2], bounds[3], 0); }

// Common entry work of the calls on a resident slot: argument checks, the stream `s` and its order, mvKeysUn.  No host wait.
static int resident_frame(orbfe_context *ctx, int slot, void *stream, hipStream_t &s, orbfe_match_device_state *&st, const KeyPointPOD *&keys)
{
    const DeviceConfig *cfg = &ctx->cfg;
    const DeviceBuffers *buf = &ctx->buf;
    if (slot < 0 || slot >= ctx->last_images)
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "device slot %d: the latest extraction call filled %d image slots", slot, ctx->last_images);
    if (cfg->sel_total > 65535) return orbfe_fail(ctx, ORBFE_ERR_UNSUPPORTED, "frames with more than 65535 keypoints are not supported by the matchers");
    st = orbfe_ctx_match_device_state(ctx);
    if (!st) return orbfe_fail(ctx, ORBFE_ERR_HIP, "out of host memory");
    const int rc = orbfe_enqueue_on(ctx, stream, true, &s); // an event wait on the stream, no host wait
    if (rc != ORBFE_OK) return rc;
    const unsigned epoch = ctx->epoch;
    const KeyPointPOD *raw = (const KeyPointPOD *)buf->kps + (size_t)slot * cfg->sel_total;
    keys = raw;
    if (cfg->n_dist > 0 && cfg->dist[0] != 0.0f) { // mvKeysUn: undistorted on the device once per frame (Frame::UndistortKeyPoints)
        const int max_images = ctx->params.max_images;
        if (st->keys_un.ensure(sizeof(KeyPointPOD) * (size_t)cfg->sel_total * max_images)) return orbfe_fail(ctx, ORBFE_ERR_HIP, "matcher scratch allocation failed");
        bool same = st->un_ndist == cfg->n_dist && (int)st->un_epoch.size() >= max_images;
        for (int k = 0; k < 5; k++) same = same && st->un_dist[k] == cfg->dist[k];
        if (!same) {
            st->un_epoch.assign(max_images, 0); // epoch 0 = no extraction call yet
            st->un_ndist = cfg->n_dist;
            for (int k = 0; k < 5; k++) st->un_dist[k] = cfg->dist[k];
        }
        KeyPointPOD *un = (KeyPointPOD *)st->keys_un.p + (size_t)slot * cfg->sel_total;
        if (st->un_epoch[slot] != epoch) {
            // the slot's count is only known on the device: every row of the slot goes through, rows past the count are never read
            orbfe_launch_undistort(*cfg, raw, un, cfg->sel_total, s);
            st->un_epoch[slot] = epoch;
            if (st->grid_slot == slot) st->grid_slot = -1; // the grid was built from other keys
        }
        keys = un;
    }
    return ORBFE_OK;
}

// the slot as the kernels read it, its grid built if this is the first call on this frame with these bounds
static int resident_grid(orbfe_context *ctx, int slot, const float *bounds, bool stereo, void *stream, hipStream_t &s, orbfe_match_device_state *&st, GridFrame &f)
{
    const DeviceConfig *cfg = &ctx->cfg;
    const DeviceBuffers *buf = &ctx->buf;
    if (!bounds || !(bounds[1] > bounds[0]) || !(bounds[3] > bounds[2])) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "bad image bounds");
    const KeyPointPOD *keys = nullptr;
    int rc = resident_frame(ctx, slot, stream, s, st, keys);
    if (rc != ORBFE_OK) return rc;
    if (st->cells.ensure(sizeof(int) * (size_t)(GRID_CELLS + 1 + cfg->sel_total))) return orbfe_fail(ctx, ORBFE_ERR_HIP, "matcher scratch allocation failed");
    const size_t so = (size_t)slot * cfg->sel_total;
    f.keys = keys;
    f.desc = buf->desc + so * 32;
    f.u_right = stereo ? buf->u_right + so : nullptr;
    f.n_ptr = buf->kp_cnt + slot;
    f.cap = cfg->sel_total;
    grid_frame_geometry(f, bounds[0], bounds[1], bounds[2], bounds[3], false); // a Frame: windows use the float bounds
    f.cell_off = (int *)st->cells.p; f.cell_idx = f.cell_off + GRID_CELLS + 1;
    const unsigned epoch = ctx->epoch;
    if (!(st->grid_epoch == epoch && st->grid_slot == slot && st->grid_keys == (const void *)f.keys && st->grid_bounds[0] == bounds[0] && st->grid_bounds[1] == bounds[1] &&
          st->grid_bounds[2] == bounds[2] && st->grid_bounds[3] == bounds[3])) {
        orbfe_launch_grid_build(f, s);
        st->grid_epoch = epoch; st->grid_slot = slot; st->grid_keys = f.keys;
        for (int k = 0; k < 4; k++) st->grid_bounds[k] = bounds[k];
    }
    return ORBFE_OK;
}

static int ensure_query_scratch(orbfe_context *ctx, orbfe_match_device_state *st, int nq)
{
    const size_t m = nq > 0 ? nq : 1;
    if (st->q.ensure(sizeof(MatchQuery) * m) || st->topk.ensure(sizeof(unsigned long long) * TOPK * m) || st->n_static.ensure(sizeof(int) * m) ||
        st->ev.ensure(sizeof(int32_t) * m))
        return orbfe_fail(ctx, ORBFE_ERR_HIP, "matcher scratch allocation failed");
    return ORBFE_OK;
}

// window query, resolution and the optional gather: what the two matchers share once their queries are written
template <class Source>
static int enqueue_window_resolve(orbfe_context *ctx, orbfe_match_device_state *st, const GridFrame &f, const Source &src, int nq, const uint8_t *d_qdesc, const int32_t *d_obs,
                                  const float *d_angle, const uint8_t *d_blocked0, int points, int check_ori, float nnratio, const float *d_pos,
                                  int32_t *d_cur_match, int32_t *d_nmatches, int32_t *d_status, uint8_t *d_has_point, float *d_Xw, hipStream_t s)
{
    const int blocks = std::max((nq + 3) / 4, (f.cap + 255) / 256); // one wave per query, and a thread per keypoint slot
    const WindowRow w = {(MatchQuery *)st->q.p, d_qdesc, nq, d_blocked0, (unsigned long long *)st->topk.p, (int *)st->n_static.p, d_cur_match};
    hipLaunchKernelGGL(window_topk_kernel<Source>, dim3(blocks), dim3(256), 0, s, f, src, w);
    ResolveArgs a;
    a.f = f; a.q = (const MatchQuery *)st->q.p; a.qdesc = d_qdesc; a.nq = nq;
    a.topk = (const unsigned long long *)st->topk.p; a.n_static = (const int *)st->n_static.p;
    a.obs = d_obs; a.angle = d_angle; a.blocked0 = d_blocked0;
    a.points = points; a.th_high = TH_HIGH; a.check_ori = check_ori; a.nnratio = nnratio; a.row_err = 0;
    a.ev = (int32_t *)st->ev.p;
    a.cur_match = d_cur_match; a.nmatches = d_nmatches; a.status = d_status;
    hipLaunchKernelGGL(resolve_kernel<OneRow>, dim3(1), dim3(RESOLVE_THREADS), 0, s, a, OneRow());
    if (d_has_point || (d_Xw && d_pos)) {
        const GatherRow g = {d_cur_match, d_pos, nullptr, d_has_point, d_Xw};
        hipLaunchKernelGGL(gather_kernel<OneRow>, dim3((f.cap + 255) / 256), dim3(256), 0, s, f, g, OneRow());
    }
    ORBFE_HIP_TRY(ctx, hipGetLastError());
    return ORBFE_OK;
}

// The keyframe matcher for n_cands candidates: four launches whatever n_cands is
static int enqueue_kf(orbfe_context *ctx, int slot, const float *bounds, const orbfe_reloc_candidate *d_cands, const orbfe_reloc_candidate &one, int n_cands,
                      int max_n, int check_ori, int exclude_held, int32_t *d_cur_match, int32_t *d_nmatches, int32_t *d_status, uint8_t *d_has_point,
                      float *d_Xw, void *stream)
{
    orbfe_match_device_state *st = nullptr;
    GridFrame f;
    hipStream_t s;
    int rc = resident_grid(ctx, slot, bounds, false, stream, s, st, f); // a plain GetFeaturesInArea: no mvuRight
    if (rc != ORBFE_OK) return rc;
    const size_t rows = (size_t)n_cands * (size_t)max_n;
    rc = ensure_query_scratch(ctx, st, (int)rows);
    if (rc != ORBFE_OK) return rc;
    if (st->found.ensure(rows ? rows : 1) || st->held.ensure((size_t)n_cands * f.cap) || st->err.ensure(sizeof(int32_t) * (size_t)n_cands))
        return orbfe_fail(ctx, ORBFE_ERR_HIP, "matcher scratch allocation failed");
    KfBatch b;
    b.V = frame_view(ctx, bounds);
    b.cands = d_cands; b.one = one; b.max_n = max_n; b.cap = f.cap; b.exclude_held = exclude_held != 0;
    b.found = (uint8_t *)st->found.p; b.held = (uint8_t *)st->held.p; b.err = (int32_t *)st->err.p;
    b.q = (MatchQuery *)st->q.p; b.topk = (unsigned long long *)st->topk.p; b.n_static = (int *)st->n_static.p; b.ev = (int32_t *)st->ev.p;
    b.cur_match = d_cur_match; b.nmatches = d_nmatches; b.status = d_status; b.has_point = d_has_point; b.Xw = d_Xw;
    hipLaunchKernelGGL(kf_prepare_kernel, dim3(n_cands), dim3(1024), 0, s, f, b);
    const int blocks = std::max((max_n + 3) / 4, (f.cap + 255) / 256);
    hipLaunchKernelGGL(window_topk_kernel<KfBatch>, dim3(blocks, n_cands), dim3(256), 0, s, f, b, WindowRow());
    ResolveArgs a = {};
    a.f = f; a.points = 0; a.check_ori = check_ori != 0; a.nnratio = 0.f; // obs stays null: every accepted keypoint is closed
    hipLaunchKernelGGL(resolve_kernel<KfBatch>, dim3(n_cands), dim3(RESOLVE_THREADS), 0, s, a, b);
    hipLaunchKernelGGL(gather_kernel<KfBatch>, dim3((f.cap + 255) / 256, n_cands), dim3(256), 0, s, f, GatherRow(), b);
    ORBFE_HIP_TRY(ctx, hipGetLastError());
    return ORBFE_OK;
}

extern "C" int orbfe_enqueue_search_by_projection_last(orbfe_context *ctx, int slot, const float *bounds, const float *d_Tcw_cur, const float *d_Tcw_last,
                                                       int n_last, const float *d_last_pos, const uint8_t *d_last_desc, const int32_t *d_last_valid,
                                                       const int32_t *d_last_obs, const int32_t *d_last_octave, const float *d_last_angle,
                                                       const uint8_t *d_cur_has_obs, float th, int mono, int check_ori, int32_t *d_cur_match,
                                                       int32_t *d_nmatches, int32_t *d_status, uint8_t *d_has_point, float *d_Xw, void *stream)
try {
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    ORBFE_ENTRY(ctx);
    if (!bounds || !d_Tcw_cur || !d_Tcw_last || !d_cur_match || !d_nmatches || !d_status || n_last < 0 ||
        (n_last > 0 && (!d_last_pos || !d_last_desc || !d_last_valid || !d_last_obs || !d_last_octave || !d_last_angle)))
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null argument");
    hipStream_t s;
    orbfe_match_device_state *st = nullptr;
    GridFrame f;
    int rc = resident_grid(ctx, slot, bounds, !mono, stream, s, st, f);
    if (rc != ORBFE_OK) return rc;
    rc = ensure_query_scratch(ctx, st, n_last);
    if (rc != ORBFE_OK) return rc;
    const LastSource src = {frame_view(ctx, bounds), d_Tcw_cur, d_Tcw_last, d_last_pos, d_last_valid, d_last_octave, th, mono};
    return enqueue_window_resolve(ctx, st, f, src, n_last, d_last_desc, d_last_obs, d_last_angle, d_cur_has_obs, 0, check_ori != 0, 0.f, d_last_pos,
                                  d_cur_match, d_nmatches, d_status, d_has_point, d_Xw, s);
} ORBFE_CATCH(ctx)

extern "C" int orbfe_enqueue_is_in_frustum(orbfe_context *ctx, const float *d_Tcw, const float *bounds, int n, const float *d_pos, const float *d_normal,
                                           const float *d_max_distance, const float *d_min_distance, float viewing_cos_limit,
                                           orbfe_track_point *d_out, void *stream)
try {
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    ORBFE_ENTRY(ctx);
    if (!d_Tcw || !bounds || n < 0 || (n > 0 && (!d_pos || !d_normal || !d_max_distance || !d_min_distance || !d_out)))
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null argument");
    if (n == 0) return ORBFE_OK;
    hipStream_t s;
    if (const int rc = orbfe_enqueue_on(ctx, stream, false, &s)) return rc;
    hipLaunchKernelGGL(frustum_kernel, dim3((n + 255) / 256), dim3(256), 0, s, frame_view(ctx, bounds), d_Tcw, n, d_pos, d_normal, d_max_distance,
                       d_min_distance, viewing_cos_limit, d_out);
    ORBFE_HIP_TRY(ctx, hipGetLastError());
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

extern "C" int orbfe_enqueue_search_by_projection_points(orbfe_context *ctx, int slot, const float *bounds, int n_pts, const orbfe_track_point *d_pts,
                                                         const uint8_t *d_pt_desc, const int32_t *d_pt_obs, const float *d_pt_pos,
                                                         const uint8_t *d_cur_has_obs, float th, float nnratio, int32_t *d_cur_match,
                                                         int32_t *d_nmatches, int32_t *d_status, uint8_t *d_has_point, float *d_Xw, void *stream)
try {
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    ORBFE_ENTRY(ctx);
    if (!bounds || !d_cur_match || !d_nmatches || !d_status || n_pts < 0 || (n_pts > 0 && (!d_pts || !d_pt_desc || !d_pt_obs)))
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null argument");
    hipStream_t s;
    orbfe_match_device_state *st = nullptr;
    GridFrame f;
    int rc = resident_grid(ctx, slot, bounds, true, stream, s, st, f);
    if (rc != ORBFE_OK) return rc;
    rc = ensure_query_scratch(ctx, st, n_pts);
    if (rc != ORBFE_OK) return rc;
    const PointsSource src = {frame_view(ctx, bounds), d_pts, th};
    return enqueue_window_resolve(ctx, st, f, src, n_pts, d_pt_desc, d_pt_obs, nullptr, d_cur_has_obs, 1, 0, nnratio, d_pt_pos, d_cur_match, d_nmatches,
                                  d_status, d_has_point, d_Xw, s);
} ORBFE_CATCH(ctx)

extern "C" int orbfe_enqueue_search_by_projection_kf(orbfe_context *ctx, int slot, const float *bounds, const float *d_Tcw, int n_kf, const float *d_kf_pos,
                                                     const uint8_t *d_kf_desc, const int32_t *d_kf_valid, const float *d_kf_angle,
                                                     const float *d_kf_max_distance, const float *d_kf_min_distance, int32_t *d_cur_point,
                                                     const uint8_t *d_outlier, float th, int orb_dist, int check_ori, int exclude_held,
                                                     int32_t *d_cur_match, int32_t *d_nmatches, int32_t *d_status, uint8_t *d_has_point, float *d_Xw,
                                                     void *stream)
try {
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    ORBFE_ENTRY(ctx);
    if (!bounds || !d_Tcw || !d_cur_point || !d_cur_match || !d_nmatches || !d_status || n_kf < 0 ||
        (n_kf > 0 && (!d_kf_pos || !d_kf_desc || !d_kf_valid || !d_kf_angle || !d_kf_max_distance || !d_kf_min_distance)))
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null argument");
    if (n_kf > (1 << 20)) return orbfe_fail(ctx, ORBFE_ERR_CAPACITY, "%d keyframe points: the matcher's scratch rows hold 2^20", n_kf);
    const orbfe_reloc_candidate one = {d_Tcw, d_kf_pos, d_kf_desc, d_kf_valid, d_kf_angle, d_kf_max_distance, d_kf_min_distance, d_cur_point, d_outlier,
                                       n_kf, th, orb_dist, 0};
    return enqueue_kf(ctx, slot, bounds, nullptr, one, 1, n_kf, check_ori, exclude_held, d_cur_match, d_nmatches, d_status, d_has_point, d_Xw,
                      stream);
} ORBFE_CATCH(ctx)

extern "C" int orbfe_enqueue_search_by_projection_kf_batch(orbfe_context *ctx, int slot, const float *bounds, const orbfe_reloc_candidate *d_cands, int n_cands,
                                                           int max_n_kf, int check_ori, int exclude_held, int32_t *d_cur_match, int32_t *d_nmatches,
                                                           int32_t *d_status, uint8_t *d_has_point, float *d_Xw, void *stream)
try {
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    ORBFE_ENTRY(ctx);
    if (!bounds || n_cands < 0 || n_cands > 65535 || max_n_kf < 0 || (n_cands > 0 && (!d_cands || !d_cur_match || !d_nmatches || !d_status)))
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null argument or count out of range");
    if (slot < 0 || slot >= ctx->last_images)
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "device slot %d: the latest extraction call filled %d image slots", slot, ctx->last_images);
    if ((long long)n_cands * max_n_kf > (1ll << 20))
        return orbfe_fail(ctx, ORBFE_ERR_CAPACITY, "%d candidates x %d points: the matcher's scratch rows hold 2^20", n_cands, max_n_kf);
    if (n_cands == 0) return ORBFE_OK;
    return enqueue_kf(ctx, slot, bounds, d_cands, orbfe_reloc_candidate(), n_cands, max_n_kf, check_ori, exclude_held, d_cur_match, d_nmatches, d_status,
                      d_has_point, d_Xw, stream);
} ORBFE_CATCH(ctx)

// ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th), src/ORBmatcher.cc:285-398, on a keyframe record: two launches
extern "C" int orbfe_enqueue_search_by_projection_sim3(orbfe_context *ctx, const orbfe_grid_keyframe *kf, const float *Scw, int n_pts, const int32_t *d_pt_index,
                                                       int n_rows, const float *d_pos, const float *d_normal, const float *d_max_distance,
                                                       const float *d_min_distance, const uint8_t *d_pt_desc, const int32_t *d_pt_valid,
                                                       const uint8_t *d_kf_matched, float th, int32_t *d_pt_match, int32_t *d_kf_match, int32_t *d_nmatches,
                                                       int32_t *d_status, void *stream)
try {
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    ORBFE_ENTRY(ctx);
    if (!kf || !Scw || !d_pt_match || !d_kf_match || !d_nmatches || !d_status) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null argument");
    Sim3Source src;
    src.pts = {{d_pt_index, n_rows, d_pos, d_normal, d_max_distance, d_min_distance, d_pt_desc, d_pt_valid}, ctx->params.nlevels, d_pt_match};
    GridFrame f;
    int rc = orbfe_point_table_frame(ctx, kf, n_pts, 1 << 20, src.pts, f); // the scratch rows hold 2^20 queries
    if (rc != ORBFE_OK) return rc;
    src.V = orbfe_view(ctx, kf);
    f.u_right = nullptr; // this matcher has no mvuRight gate: kf->u_right is never read
    orbfe_match_device_state *st = orbfe_ctx_match_device_state(ctx);
    if (!st) return orbfe_fail(ctx, ORBFE_ERR_HIP, "out of host memory");
    hipStream_t s;
    rc = orbfe_enqueue_on(ctx, stream, false, &s);
    if (rc != ORBFE_OK) return rc;
    rc = ensure_query_scratch(ctx, st, n_pts);
    if (rc != ORBFE_OK) return rc;
    src.kf_n = kf->n;
    orbfe_resolve::sim3_to_rt(Scw, src.T);
    orbfe_resolve::camera_center(src.T, src.ow);
    src.th = th;
    // one wave per query, and a thread per keypoint for the reset of d_kf_match; neither: the resolve kernel alone writes count and status
    const int blocks = std::max((n_pts + 3) / 4, (f.cap + 255) / 256);
    const WindowRow w = {(MatchQuery *)st->q.p, nullptr, n_pts, d_kf_matched, (unsigned long long *)st->topk.p, (int *)st->n_static.p, d_kf_match};
    if (blocks > 0) hipLaunchKernelGGL((window_topk_kernel<Sim3Source, true>), dim3(blocks), dim3(256), 0, s, f, src, w);
    ResolveArgs a = {};
    a.f = f; a.q = (const MatchQuery *)st->q.p; a.nq = n_pts;
    a.topk = (const unsigned long long *)st->topk.p; a.n_static = (const int *)st->n_static.p;
    a.blocked0 = d_kf_matched; // obs stays null: every accepted keypoint is closed (vpMatched[bestIdx] = pMP, :390)
    a.th_high = TH_LOW;        // no ratio, no rotation test
    a.ev = (int32_t *)st->ev.p;
    a.cur_match = d_kf_match; a.nmatches = d_nmatches; a.status = d_status;
    hipLaunchKernelGGL((resolve_kernel<Sim3Points, true>), dim3(1), dim3(RESOLVE_THREADS), 0, s, a, src.pts);
    ORBFE_HIP_TRY(ctx, hipGetLastError());
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

extern "C" int orbfe_device_keys_un(orbfe_context *ctx, int slot, const orbfe_keypoint **d_keys_un, void *stream)
try {
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    ORBFE_ENTRY(ctx);
    if (!d_keys_un) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null argument");
    hipStream_t s;
    orbfe_match_device_state *st = nullptr;
    const KeyPointPOD *keys = nullptr;
    const int rc = resident_frame(ctx, slot, stream, s, st, keys);
    if (rc != ORBFE_OK) return rc;
    ORBFE_HIP_TRY(ctx, hipGetLastError());
    *d_keys_un = (const orbfe_keypoint *)keys;
    return ORBFE_OK;
} ORBFE_CATCH(ctx)
