// orbfe_match_window.hpp -- the device statements the Tracking matchers share below their resolution: the frame grid
// (Frame::PosInGrid), the window of a query (Frame::GetFeaturesInArea), the walk over its keypoints, the candidate key and the
// selection of a query's four smallest keys.  orbfe_match.hip (candidate lists for the host replay) and orbfe_match_device.hip
// (resolution on the device) both include it, so every statement of the bit-exactness contracts -- Q4 (no FMA contraction, no
// fast-math), Q5 (the level check), Q6 (round(), column 64 dropped) -- and the key layout
//      dist << 36 | ix << 30 | iy << 24 | idx << 8 | octave        (dist 511: failed the mvuRight gate)
// exists once; so do the view of a context (orbfe_view), the table of candidate map points of the keyframe-side matchers (PointTable)
// and their search without greedy state (wave_best_key).  Only __device__ __forceinline__ functions, host helpers, structs and constants: the library has no relocatable device code, so
// the one kernel over these (grid_build_kernel, orbfe_match_device.hip) is reached through orbfe_launch_grid_build.
#pragma once

#include "orbfe_common.hpp"
#include "orbfe_host.h"
#include "orbfe_match_resolve.h"

#define GRID_COLS 64 // FRAME_GRID_COLS include/Frame.h:36
#define GRID_ROWS 48 // FRAME_GRID_ROWS include/Frame.h:37
#define GRID_CELLS (GRID_COLS * GRID_ROWS)
#define NO_KEY (~0ull)

// a frame as the kernels see it
struct GridFrame {
    const KeyPointPOD *keys; // mvKeysUn
    const uint8_t *desc;
    const float *u_right;    // null: no mvuRight gate
    const int *n_ptr;        // the keypoint counter of a resident slot (DeviceBuffers::kp_cnt); null: the frame holds `cap` keypoints
    int cap;                 // keypoint capacity of the slot, or the count of an uploaded frame
    float min_x, min_y, inv_w, inv_h; // Frame::mnMinX / mnMinY, mfGridElementWidthInv / HeightInv: the grid ASSIGNMENT
    float q_min_x, q_min_y;           // bounds of the window QUERY: the same, or (float)(int) of them for a KeyFrame (src/KeyFrame.cc:568-580)
    int *cell_off, *cell_idx;         // CSR over ix * GRID_ROWS + iy
};

// The geometry of a GridFrame from the frame's float bounds, on the host, for every path that builds one: cells are assigned with the
// floats (mfGridElementWidthInv / HeightInv, src/Frame.cc:99-100); a KeyFrame's windows use (float)(int) of the lower bounds
// (KeyFrame::mnMinX is an int initialised from the frame's float, src/KeyFrame.cc:568-580)
static inline void grid_frame_geometry(GridFrame &f, float min_x, float max_x, float min_y, float max_y, bool keyframe)
{
    f.min_x = min_x; f.min_y = min_y;
    f.inv_w = (float)GRID_COLS / (max_x - min_x);
    f.inv_h = (float)GRID_ROWS / (max_y - min_y);
    f.q_min_x = keyframe ? (float)(int)min_x : min_x;
    f.q_min_y = keyframe ? (float)(int)min_y : min_y;
}

// The context's view (orbfe_match_resolve.h) with these bounds, or with those of a frame view / keyframe record
static inline orbfe_resolve::View orbfe_view(orbfe_context *ctx, float min_x, float max_x, float min_y, float max_y, int keyframe)
{
    return orbfe_resolve::view_of(&ctx->params, ctx->plan.scale, min_x, max_x, min_y, max_y, keyframe);
}
template <class Record> // orbfe_frame_view, orbfe_grid_keyframe
static inline orbfe_resolve::View orbfe_view(orbfe_context *ctx, const Record *r)
{
    return orbfe_view(ctx, r->min_x, r->max_x, r->min_y, r->max_y, r->keyframe != 0);
}

// The table of candidate map points of Fuse and of the Sim3 SearchByProjection on a keyframe record: n_rows rows in device memory,
// query q reading row q or, through an index list, row pt_index[q].  pt_valid is per query, everything else per row.
struct PointTable {
    const int32_t *pt_index; // null: query q is row q (n_rows >= the query count: the call checked it)
    int n_rows;
    const float *pos, *normal, *max_distance, *min_distance;
    const uint8_t *pt_desc;
    const int32_t *pt_valid;
    // the row of query q, tested before it addresses the table; -1: outside [0, n_rows)
    __device__ __forceinline__ int row(int q) const
    {
        if (!pt_index) return q;
        const int r = pt_index[q];
        return (r < 0 || r >= n_rows) ? -1 : r;
    }
    __device__ __forceinline__ const uint8_t *desc(int q) const // only followed for a query with a window, whose row is good
    {
        const int r = row(q);
        return pt_desc + (size_t)(r < 0 ? 0 : r) * 32;
    }
};
// What a call refuses about n_pts queries over table t against keyframe record kf (max_pts: what its scratch holds), and kf as the
// kernels read it (orbfe_fuse_device.hip)
int orbfe_point_table_frame(orbfe_context *ctx, const orbfe_grid_keyframe *kf, int n_pts, int max_pts, const PointTable &t, GridFrame &f);

__device__ __forceinline__ int frame_count(const GridFrame &f)
{
    if (!f.n_ptr) return f.cap;
    const int n = *f.n_ptr;
    return n < 0 ? 0 : (n > f.cap ? f.cap : n);
}
// Frame::PosInGrid (src/Frame.cc:383-393; Q6: round(), column 64 dropped)
__device__ __forceinline__ int grid_cell(const GridFrame &f, int i)
{
    const int px = (int)roundf(__fmul_rn(__fsub_rn(f.keys[i].x, f.min_x), f.inv_w));
    const int py = (int)roundf(__fmul_rn(__fsub_rn(f.keys[i].y, f.min_y), f.inv_h));
    return (px >= 0 && px < GRID_COLS && py >= 0 && py < GRID_ROWS) ? px * GRID_ROWS + py : -1;
}

// The cells of a query's window (Frame::GetFeaturesInArea, src/Frame.cc:328-381)
struct Window { int min_cx, min_cy, ncy, ncells; };
__device__ __forceinline__ Window query_window(const GridFrame &f, const orbfe_resolve::MatchQuery &Q)
{
    Window w = {0, 0, 1, 0};
    if (!(Q.flags & 1)) return w;
    int v = (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(Q.u, f.q_min_x), Q.r), f.inv_w));
    w.min_cx = v > 0 ? v : 0;
    v = (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(Q.u, f.q_min_x), Q.r), f.inv_w));
    const int max_cx = v < GRID_COLS - 1 ? v : GRID_COLS - 1;
    v = (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(Q.v, f.q_min_y), Q.r), f.inv_h));
    w.min_cy = v > 0 ? v : 0;
    v = (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(Q.v, f.q_min_y), Q.r), f.inv_h));
    const int max_cy = v < GRID_ROWS - 1 ? v : GRID_ROWS - 1;
    if (w.min_cx < GRID_COLS && max_cx >= 0 && w.min_cy < GRID_ROWS && max_cy >= 0 && max_cx >= w.min_cx && max_cy >= w.min_cy) {
        w.ncy = max_cy - w.min_cy + 1;
        w.ncells = (max_cx - w.min_cx + 1) * w.ncy;
    }
    return w;
}

// Calls fn(ix, iy, idx, kp) for every keypoint of the window this lane owns (cells lane, lane + 64, ...) that passes the level
// and radius tests.
// CHECKED is for a grid and keypoints that the caller uploaded (orbfe_grid_keyframe) instead of grid_build_kernel and the extraction:
// a cell's offsets must lie in 0 <= begin <= end <= n, an index in [0, n) and a keypoint's octave in [0, nlevels), each tested before
// it is used as an address (the octave indexes the caller's level tables); what fails is skipped and the walk returns false.  The
// octave is tested on every keypoint of a walked cell, before the level test drops it.  Unchecked, the walk is as it always was.
template <bool CHECKED = false, class Fn>
__device__ __forceinline__ bool for_each_hit(const GridFrame &f, const orbfe_resolve::MatchQuery &Q, const Window &w, int lane, Fn fn, int n = 0, int nlevels = 0)
{
    const bool check_levels = (Q.min_level > 0) || (Q.max_level >= 0); // Q5, literally
    bool ok = true;
    for (int c = lane; c < w.ncells; c += 64) {
        const int ix = w.min_cx + c / w.ncy, iy = w.min_cy + c % w.ncy;
        const int cell = ix * GRID_ROWS + iy;
        int begin = 0, end = 0;
        if constexpr (CHECKED) {
            begin = f.cell_off[cell];
            end = f.cell_off[cell + 1];
            if (begin < 0 || end < begin || end > n) { ok = false; continue; }
        }
#pragma unroll 1 // a counting fn would otherwise be unrolled 16 deep: a cell holds a keypoint or two, and the registers cost occupancy
        for (int j = CHECKED ? begin : f.cell_off[cell]; j < (CHECKED ? end : f.cell_off[cell + 1]); j++) {
            const int idx = f.cell_idx[j];
            if constexpr (CHECKED)
                if (idx < 0 || idx >= n) { ok = false; continue; }
            const KeyPointPOD kp = f.keys[idx];
            if constexpr (CHECKED)
                if (kp.octave < 0 || kp.octave >= nlevels) { ok = false; continue; }
            if (check_levels && (kp.octave < Q.min_level || (Q.max_level >= 0 && kp.octave > Q.max_level))) continue;
            if (!(fabsf(__fsub_rn(kp.x, Q.u)) < Q.r && fabsf(__fsub_rn(kp.y, Q.v)) < Q.r)) continue;
            fn(ix, iy, idx, kp);
        }
    }
    return ok;
}
// The key of a hit: the Hamming distance to the query descriptor qd over the hit's place in GetFeaturesInArea order
__device__ __forceinline__ unsigned long long candidate_key(const GridFrame &f, const orbfe_resolve::MatchQuery &Q, const uint32_t (&qd)[8], int ix, int iy, int idx,
                                                            const KeyPointPOD &kp)
{
    unsigned dist = 0;
    const uint32_t *p = (const uint32_t *)(f.desc + (size_t)idx * 32);
#pragma unroll
    for (int k = 0; k < 8; k++) dist += __popc(qd[k] ^ p[k]);
    // the mvuRight gate (src/ORBmatcher.cc:93-98,1403-1409) is a pure function of the pair: mark it
    if ((Q.flags & 2) && f.u_right && f.u_right[idx] > 0 && fabsf(__fsub_rn(Q.ur, f.u_right[idx])) > Q.ur_rad) dist = 511;
    return ((unsigned long long)dist << 36) | ((unsigned long long)ix << 30) | ((unsigned long long)iy << 24) | ((unsigned long long)idx << 8) |
           (unsigned long long)(kp.octave & 255);
}
// emit(key, idx) for every hit of the lane; CHECKED, n and nlevels as for_each_hit, whose verdict is returned
template <bool CHECKED = false, class Emit>
__device__ __forceinline__ bool scan_window(const GridFrame &f, const orbfe_resolve::MatchQuery &Q, const Window &w, const uint32_t *__restrict__ qdesc, int lane, Emit emit,
                                            int n = 0, int nlevels = 0)
{
    uint32_t qd[8];
#pragma unroll
    for (int k = 0; k < 8; k++) qd[k] = qdesc[k];
    return for_each_hit<CHECKED>(f, Q, w, lane, [&](int ix, int iy, int idx, const KeyPointPOD &kp) { emit(candidate_key(f, Q, qd, ix, iy, idx, kp), idx); }, n, nlevels);
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long w)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)w, o, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(w >> 32), o, 64);
        const unsigned long long t = ((unsigned long long)hi << 32) | lo;
        w = t < w ? t : w;
    }
    return w;
}

// Search without greedy state (Fuse, SearchBySim3: the points do not interact), one wave per query over a caller's keyframe record:
// the checked walk of Q's window (n, nlevels as for_each_hit), gate(idx, kp) per hit, and the wave's smallest key = the reference
// loop's first minimum (NO_KEY: none).  clean: the walk of every lane was.  Whole waves call it.
template <class Gate>
__device__ __forceinline__ unsigned long long wave_best_key(const GridFrame &f, const orbfe_resolve::MatchQuery &Q, const uint8_t *qdesc, int lane, Gate gate, int n,
                                                            int nlevels, bool &clean)
{
    unsigned long long best = NO_KEY;
    bool ok = true;
    const Window w = query_window(f, Q);
    if (w.ncells > 0) {
        uint32_t qd[8];
#pragma unroll
        for (int k = 0; k < 8; k++) qd[k] = ((const uint32_t *)qdesc)[k];
        ok = for_each_hit<true>(
            f, Q, w, lane,
            [&](int ix, int iy, int idx, const KeyPointPOD &kp) {
                if (!gate(idx, kp)) return; // kp.octave lies in [0, nlevels): the checked walk has tested it
                const unsigned long long key = candidate_key(f, Q, qd, ix, iy, idx, kp);
                if (key < best) best = key;
            },
            n, nlevels);
    }
    clean = __all(ok) != 0;
    return wave_min_u64(best);
}

// The four smallest keys a lane has seen, ascending, in registers; the wave merges its lanes' four by four pops: any window size
struct Top4 {
    unsigned long long t0 = NO_KEY, t1 = NO_KEY, t2 = NO_KEY, t3 = NO_KEY;
    __device__ __forceinline__ void insert(unsigned long long key)
    {
        if (key < t3) {
            t3 = key;
            if (t3 < t2) { const unsigned long long x = t2; t2 = t3; t3 = x; }
            if (t2 < t1) { const unsigned long long x = t1; t1 = t2; t2 = x; }
            if (t1 < t0) { const unsigned long long x = t0; t0 = t1; t1 = x; }
        }
    }
    // the smallest key left in the wave (NO_KEY: none); keys are unique within a query (they carry the keypoint index), so exactly one lane retires it
    __device__ __forceinline__ unsigned long long pop_wave_min()
    {
        const unsigned long long m = wave_min_u64(t0);
        if (m != NO_KEY && t0 == m) { t0 = t1; t1 = t2; t2 = t3; t3 = NO_KEY; }
        return m;
    }
};
