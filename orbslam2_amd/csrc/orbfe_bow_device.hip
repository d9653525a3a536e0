// orbfe_bow_device.hip -- Frame::ComputeFboW (src/Frame.cc:395-400; fbow transform, Thirdparty/fbow/src/fbow.h:400-444) and
// ORBmatcher::SearchByFboW(KeyFrame*, Frame&) (src/ORBmatcher.cc:157-283) on a device-resident frame, asynchronous on the
// caller's stream: device pointers in, results in HBM, no host wait.  orbfe_bow.hip is the synchronous form (descriptors
// uploaded again, maps and greedy resolve on the host) and the second implementation this one is tested against.
//
// orbfe_enqueue_compute_bow, three launches sized by the keypoint capacity (the slot's count is only known on the device):
//   bow_descend_resident_kernel  bow_walk per descriptor; word id, node id and weight of feature f go to entry f of HBM scratch
//   bow_rank_kernel              sorts the keys (id << 32 | feature) of both maps by rank: a key's place is the number of smaller
//                                keys.  The feature half of key f is f, its position, so only the 32-bit ids are staged in LDS
//                                (tiles of BOW_RANK_TILE) and compared.  Keys are unique, so the ranks are a permutation and the
//                                features inside a word / node ascend.  One tile covers a usual frame; above that the kernel walks
//                                the id array in HBM scratch tile by tile, up to the capacity.
//   bow_segments_kernel          one workgroup per map: segment heads -> scan -> CSR.  A word's weights are added by ONE thread in
//                                feature order (fbow.h:431): a tree sum rounds differently.
// orbfe_enqueue_search_by_bow, three launches:
//   bow_match_init_kernel        f_match = -1 below the slot's count, d_status
//   bow_node_match_kernel        one wave per keyframe node.  A frame keypoint lies in one node of the frame's feature vector and
//                                the greedy rule of :203-229 only skips frame keypoints matched earlier, so it is sequential only
//                                inside a node: the wave takes the node's KF features in order, its lanes stride over the node's
//                                frame features, and the "already matched" flags of a lane's features stay in that lane's registers.
//                                This is bow_shared_node (the merge-join step: checks, then the 64-way probe) and bow_node_walk<Side>,
//                                shared with the (KeyFrame, KeyFrame) overload; a Side states what differs between the two.
//   bow_match_tail_kernel        the rotation histogram needs every node: bins, ComputeThreeMaxima, losers removed, the count,
//                                and the optional has_point / Xw for orbfe_enqueue_pose_optimization
// orbfe_enqueue_search_by_bow_batch (Relocalization, src/Tracking.cc:1445-1476: the candidates are independent), the same three
// launches for all keyframes: bow_*_batch_kernel run the same device functions on a BowSearch built from record blockIdx.y
// (tail: blockIdx.x) of the caller's orbfe_bow_keyframe array and that row of the outputs.
// orbfe_enqueue_search_for_triangulation (ORBmatcher::SearchForTriangulation, src/ORBmatcher.cc:652-819; the synchronous form is in
// orbfe_bow.hip), both keyframes device-resident, three launches:
//   tri_init_kernel              match12 = -1, status, count
//   tri_node_match_kernel        one wave per KF1 node: the sweep of KF2's node list and bow_shared_node, then a loop of its own, the
//                                shape of bow_node_walk with the acceptance rule of :712-750: Hamming <= TH_LOW, then the gates -- epipole
//                                disc, CheckDistEpipolarLine (orbfe_epipolar.h) --, last of the equal minima, no ratio test
//   tri_tail_kernel              match12_tail: rotation histogram, ComputeThreeMaxima, the count, vMatchedPairs by an ordered compaction
// One call per neighbour, never a batch: CreateNewMapPoints adds points to KF1 between two neighbours.
// orbfe_enqueue_search_by_bow_kf / _batch (ORBmatcher::SearchByFboW(KeyFrame*, KeyFrame*), src/ORBmatcher.cc:517-650; the synchronous form
// is in orbfe_bow.hip), both keyframes device-resident, three launches for all candidates of LoopClosing::ComputeSim3:
//   bowkf_init_kernel            rows of match12 = -1, count, status
//   bowkf_node_match_kernel      one wave per (KF1 node, candidate): sweep, bow_shared_node and bow_node_walk with BowKfSide: KF1 as the
//                                query side, valid2 on the candidates, the flag on the KF2 side and the strict bound
//   bowkf_tail_kernel            match12_tail, the tail tri_tail_kernel runs
#include "../../include/orbfe.h"
#include "orbfe_device.h"
#include "orbfe_host.h"
#include "orbfe_common.hpp"
#include "orbfe_bow_vocab.h"
#include "orbfe_match_resolve.h"
#include "orbfe_epipolar.h"

#include <cmath>

using orbfe_resolve::HISTO_LENGTH;
using orbfe_resolve::TH_LOW;

#define BOW_RANK_TILE 4096 // ids per LDS tile of bow_rank_kernel: 16 KB
#define BOW_SEG_LDS 4096   // entries per map that bow_segments_kernel stages in LDS: 32 KB
#define BOW_REG_CHUNKS 2   // a lane keeps the descriptors of its first two features of a node in registers (nodes up to 128 features)
#define BOW_FLAG_CHUNKS 64 // a lane keeps the flags of its first 64 features of a node in one 64-bit register (nodes up to 4096 features)

__device__ __forceinline__ int slot_count(const int *n_ptr, int cap)
{
    const int n = *n_ptr;
    return n < 0 ? 0 : (n > cap ? cap : n);
}

// ---------------------------------------------------------------------------------------------
// ComputeFboW
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bow_descend_resident_kernel(BowTree t, int store_level, const uint8_t *__restrict__ desc, const int *__restrict__ n_ptr, int cap,
                                                                   uint32_t *__restrict__ word_id, float *__restrict__ weight, uint32_t *__restrict__ node_id,
                                                                   uint32_t *__restrict__ id_w, uint32_t *__restrict__ id_n, float *__restrict__ wt, int32_t *__restrict__ status)
{
    const int n = slot_count(n_ptr, cap);
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f == 0) *status = n > 0 ? ORBFE_OK : ORBFE_ERR_INVALID; // fbow: "Vocabulary::transform No input data"
    if (f >= n) return;
    uint32_t wid, nid;
    float w;
    bow_walk(t, store_level, desc + (size_t)32 * f, wid, w, nid);
    if (word_id) word_id[f] = wid;
    if (weight) weight[f] = w;
    if (node_id) node_id[f] = nid;
    id_w[f] = wid; id_n[f] = nid; wt[f] = w;
}

// How many of 16 ids are below `mid` (LE: or equal to it)
template <bool LE>
__device__ __forceinline__ int count_below(const uint4 *__restrict__ v4, uint32_t mid)
{
    int c = 0;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const uint4 v = v4[u];
        c += LE ? (int)(v.x <= mid) + (int)(v.y <= mid) + (int)(v.z <= mid) + (int)(v.w <= mid)
                : (int)(v.x < mid) + (int)(v.y < mid) + (int)(v.z < mid) + (int)(v.w < mid);
    }
    return c;
}

// blockIdx.y = 0: the word keys, 1: the node keys (ids / sorted_id / sorted_pay hold both maps, `cap` entries apart).  A
// workgroup ranks 64 keys, its four waves each against a quarter of every tile:
//      key j < key i  <=>  id_j <= id_i for j < i, id_j < id_i for j > i.
// What travels with a key to its place: a word's weight, a node's feature index.
__global__ __launch_bounds__(256) void bow_rank_kernel(const uint32_t *__restrict__ ids, const float *__restrict__ wt, uint32_t *__restrict__ sorted_id,
                                                       uint32_t *__restrict__ sorted_pay, const int *__restrict__ n_ptr, int cap)
{
    __shared__ uint4 s_id[BOW_RANK_TILE / 4];
    __shared__ int s_part[4][64];
    const int n = slot_count(n_ptr, cap);
    if ((int)blockIdx.x * 64 >= n) return; // the whole workgroup
    const uint32_t *k = ids + (size_t)blockIdx.y * cap;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = blockIdx.x * 64 + lane;
    const uint32_t mid = i < n ? k[i] : 0xffffffffu;
    int rank = 0;
    for (int base = 0; base < n; base += BOW_RANK_TILE) {
        const int cnt = n - base < BOW_RANK_TILE ? n - base : BOW_RANK_TILE;
        if (base) __syncthreads();
        // the padding (last tile only, positions beyond every feature) is never below an id
#pragma unroll
        for (int u = 0; u < BOW_RANK_TILE / 256; u++) {
            const int j = tid + 256 * u;
            ((uint32_t *)s_id)[j] = j < cnt ? k[base + j] : 0xffffffffu;
        }
        __syncthreads();
        const int li = i - base; // this thread's own position in the tile (beyond it: a later tile, negative: an earlier one)
        const int steps = (cnt + 15) >> 4, per = (steps + 3) >> 2; // 16 ids per step, the steps of this tile split evenly over the waves
        const int s1 = (wave + 1) * per < steps ? (wave + 1) * per : steps;
        for (int s = wave * per; s < s1; s++) { // every lane reads the same address: a broadcast
            const int j0 = 16 * s;
            if (j0 + 16 <= li) rank += count_below<true>(s_id + 4 * s, mid);
            else if (j0 >= li) rank += count_below<false>(s_id + 4 * s, mid);
            else { // the step holds this thread's own key
#pragma unroll
                for (int u = 0; u < 16; u++) {
                    const uint32_t v = ((const uint32_t *)s_id)[j0 + u];
                    rank += j0 + u < li ? (int)(v <= mid) : (int)(v < mid);
                }
            }
        }
    }
    s_part[wave][lane] = rank;
    __syncthreads();
    if (wave == 0 && i < n) {
        const size_t r = (size_t)blockIdx.y * cap + s_part[0][lane] + s_part[1][lane] + s_part[2][lane] + s_part[3][lane]; // n distinct keys: rank < n
        sorted_id[r] = mid;
        sorted_pay[r] = blockIdx.y == 0 ? __float_as_uint(wt[i]) : (uint32_t)i;
    }
}
static_assert(BOW_RANK_TILE % 256 == 0, "bow_rank_kernel: every thread stages the same number of ids, a quarter of the tile is whole 16-id steps");

// blockIdx.x = 0: fBow (words, summed weights), 1: fBow2 (nodes -> features).  A usual frame (up to BOW_SEG_LDS keypoints) is staged
// in LDS in one batch of loads, 32 KB; a larger one is read in place.
__global__ __launch_bounds__(1024) void bow_segments_kernel(const uint32_t *__restrict__ sorted_id, const uint32_t *__restrict__ sorted_pay,
                                                            const int *__restrict__ n_ptr, int cap,
                                                            uint32_t *__restrict__ words, float *__restrict__ word_w, int32_t *__restrict__ n_words,
                                                            uint32_t *__restrict__ nodes, int32_t *__restrict__ node_off, int32_t *__restrict__ node_feat,
                                                            int32_t *__restrict__ n_nodes)
{
    __shared__ uint32_t s_id[BOW_SEG_LDS], s_pay[BOW_SEG_LDS];
    __shared__ int s_wave[16];
    const int n = slot_count(n_ptr, cap);
    const int tid = threadIdx.x, which = blockIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t *id = sorted_id + (size_t)which * cap, *pay = sorted_pay + (size_t)which * cap;
    if (n <= BOW_SEG_LDS) {
#pragma unroll
        for (int u = 0; u < BOW_SEG_LDS / 1024; u++) {
            const int j = tid + 1024 * u;
            if (j < n) { s_id[j] = id[j]; s_pay[j] = pay[j]; }
        }
        id = s_id; pay = s_pay;
        __syncthreads();
    }
    const int chunk = (n + 1023) / 1024;
    const int lo = tid * chunk < n ? tid * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
    int heads = 0;
    for (int p = lo; p < hi; p++) heads += p == 0 || id[p - 1] != id[p];
    int incl = heads; // inclusive scan inside the wave, then over the 16 wave totals
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < 16; w++) {
        const int t = s_wave[w];
        before += w < wave ? t : 0;
        total += t;
    }
    int seg = before + incl - heads;
    for (int p = lo; p < hi; p++) {
        const uint32_t v = id[p];
        const bool head = p == 0 || id[p - 1] != v;
        if (which == 0) {
            if (!head) continue;
            float sum = 0.f; // std::map's value-initialised float, then += in feature order
            for (int q = p; q < n && id[q] == v; q++) sum = __fadd_rn(sum, __uint_as_float(pay[q]));
            words[seg] = v; word_w[seg] = sum;
            seg++;
        } else {
            node_feat[p] = (int32_t)pay[p];
            if (head) { nodes[seg] = v; node_off[seg] = p; seg++; }
        }
    }
    if (tid == 0) {
        if (which == 0) *n_words = total;
        else {
            *n_nodes = total;
            if (n > 0) node_off[total] = n;
        }
    }
}
static_assert(BOW_SEG_LDS % 1024 == 0, "bow_segments_kernel: every thread stages the same number of entries");

extern "C" int orbfe_enqueue_compute_bow(orbfe_context *ctx, int slot, int level, uint32_t *d_word_id, float *d_weight, uint32_t *d_node_id,
                                         uint32_t *d_words, float *d_word_w, int32_t *d_n_words,
                                         uint32_t *d_nodes, int32_t *d_node_off, int32_t *d_node_feat, int32_t *d_n_nodes,
                                         int32_t *d_status, void *stream)
try {
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    ORBFE_ENTRY(ctx);
    if (level < 0 || !d_words || !d_word_w || !d_n_words || !d_nodes || !d_node_off || !d_node_feat || !d_n_nodes || !d_status)
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null argument");
    orbfe_bow_state *st = orbfe_ctx_bow_state(ctx);
    if (!st || !st->loaded) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "no vocabulary loaded (orbfe_vocab_load)");
    const DeviceConfig *cfg = &ctx->cfg;
    const DeviceBuffers *buf = &ctx->buf;
    if (slot < 0 || slot >= ctx->last_images)
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "device slot %d: the latest extraction call filled %d image slots", slot, ctx->last_images);
    const int cap = cfg->sel_total;
    if (cap <= 0 || cap > 65535) return orbfe_fail(ctx, ORBFE_ERR_UNSUPPORTED, "frames with more than 65535 keypoints are not supported");
    hipStream_t s;
    const int rc = orbfe_enqueue_on(ctx, stream, true, &s); // an event wait on the stream, no host wait
    if (rc != ORBFE_OK) return rc;
    if (st->resident.ensure((size_t)cap * 7 * sizeof(uint32_t))) return orbfe_fail(ctx, ORBFE_ERR_HIP, "BoW scratch allocation failed");
    uint32_t *ids = (uint32_t *)st->resident.p, *sorted_id = ids + 2 * (size_t)cap, *sorted_pay = sorted_id + 2 * (size_t)cap; // [2][cap] each: words, nodes
    float *wt = (float *)(sorted_pay + 2 * (size_t)cap);
    const BowTree t = {st->d_data, (unsigned)st->p.block_size_bytes_wp, (unsigned)st->p.feature_off_start, (unsigned)st->p.child_off_start,
                       (unsigned)st->p.desc_size_bytes_wp, (int)ceil(log2((double)st->p.m_k))};
    const uint8_t *desc = buf->desc + (size_t)slot * cap * 32;
    const int *n_ptr = buf->kp_cnt + slot;
    hipLaunchKernelGGL(bow_descend_resident_kernel, dim3((cap + 255) / 256), dim3(256), 0, s, t, level, desc, n_ptr, cap, d_word_id, d_weight, d_node_id, ids, ids + cap,
                       wt, d_status);
    hipLaunchKernelGGL(bow_rank_kernel, dim3((cap + 63) / 64, 2), dim3(256), 0, s, (const uint32_t *)ids, (const float *)wt, sorted_id, sorted_pay, n_ptr, cap);
    hipLaunchKernelGGL(bow_segments_kernel, dim3(2), dim3(1024), 0, s, (const uint32_t *)sorted_id, (const uint32_t *)sorted_pay, n_ptr, cap, d_words, d_word_w,
                       d_n_words, d_nodes, d_node_off, d_node_feat, d_n_nodes);
    ORBFE_HIP_TRY(ctx, hipGetLastError());
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

// ---------------------------------------------------------------------------------------------
// SearchByFboW(KeyFrame*, Frame&)
// ---------------------------------------------------------------------------------------------
struct BowSearch {
    const uint32_t *kf_nodes; const int32_t *kf_off, *kf_feat; int kf_nnodes;   // the keyframe's feature vector (CSR)
    const int32_t *kf_valid; const uint8_t *kf_desc; const float *kf_angle; int n_kf;
    const float *kf_pos;                                                        // optional, for Xw
    const uint32_t *f_nodes; const int32_t *f_off, *f_feat, *f_n_nodes;         // the frame's, as orbfe_enqueue_compute_bow wrote it
    const KeyPointPOD *keys; const uint8_t *desc; const int *n_ptr; int cap;    // the slot
    float nnratio; int check_ori;
    int32_t *match, *nmatches, *status;
    uint8_t *has_point; float *Xw;
};

__device__ __forceinline__ void bow_match_init(const BowSearch &a)
{
    const int n = slot_count(a.n_ptr, a.cap);
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k == 0) *a.status = n > 0 ? ORBFE_OK : ORBFE_ERR_INVALID; // a frame without keypoints has no BoW vector to search by
    if (k < n) a.match[k] = -1;
}

// First of the n ascending node ids that is >= id (n: none), by the whole wave: the lanes probe 64 places at once, the range
// shrinks 64-fold per load.
__device__ __forceinline__ int bow_lower_bound(const uint32_t *__restrict__ nodes, int n, uint32_t id, int lane)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int step = (hi - lo + 63) >> 6;
        const int p = lo + lane * step;
        const int c = __popcll(__ballot(p < hi && nodes[p] < id)); // probes below id: a prefix of the lanes
        if (c == 0) { hi = lo; break; }
        const int top = lo + c * step;
        lo += (c - 1) * step + 1;
        hi = top < hi ? top : hi;
    }
    return lo;
}

// One side of a node merge-join as a kernel holds it: the ascending node ids, the CSR offsets into the feature list, and the
// length n of the keypoint array, which no CSR exceeds (a keypoint lies in one node).
struct BowNodes {
    const uint32_t *nodes; const int32_t *off; int nnodes, n;
};

// The merge-join step (:173-282, :537-616, :676-806) of one wave: node `node` of the query side q and the node of the same id on the
// candidate side c.  In this order: q's node id strictly above its predecessor (std::map order, which the merge-join relies on) and
// its CSR range inside [0, q.n); the 64-way probe of c's node list; that node's CSR range inside [0, c.n).  A record that fails a
// check is reported in *status; false is "nothing to do": refused, past q's list, an id on one side only, or an empty range.
// EAGER: q's four entries are loaded side by side, the predecessor's id whether or not it is needed, and compared without a branch
// between them.  It is for bow_node_match_batch_kernel alone, whose keyframe arrays are pointers read from a record: its loads of q
// are flat loads that the compiler otherwise puts off, one behind the other's comparison (DESIGN.md §4e has the figures).  Where the
// pointers are kernel arguments the form without EAGER, the one the three kernels had, is the faster one.
template <bool EAGER>
__device__ __forceinline__ bool bow_shared_node(const BowNodes &q, const BowNodes &c, int node, int lane, int32_t *status, int &k0, int &k1, int &f0, int &nf)
{
    if (node >= q.nnodes) return false;
    const uint32_t id = q.nodes[node];
    k0 = q.off[node]; k1 = q.off[node + 1];
    bool refused;
    if (EAGER) {
        const uint32_t before = q.nodes[node > 0 ? node - 1 : 0];
        refused = (node > 0 && before >= id) | (k0 < 0) | (k1 < k0) | (k1 > q.n);
    } else refused = (node > 0 && q.nodes[node - 1] >= id) || k0 < 0 || k1 < k0 || k1 > q.n;
    if (refused) {
        if (lane == 0) *status = ORBFE_ERR_INVALID;
        return false;
    }
    const int lo = bow_lower_bound(c.nodes, c.nnodes, id, lane);
    if (lo >= c.nnodes || c.nodes[lo] != id) return false;
    f0 = c.off[lo];
    const int f1 = c.off[lo + 1];
    if (f0 < 0 || f1 < f0 || f1 > c.n) {
        if (lane == 0) *status = ORBFE_ERR_INVALID;
        return false;
    }
    nf = f1 - f0;
    return k1 > k0 && nf > 0;
}

// The candidate side's whole node list and CSR, once over the grid's x axis, for a side that the caller wrote (the frame's is
// orbfe_enqueue_compute_bow's): the probe above assumes ascending ids whatever node it lands on.
__device__ __forceinline__ void bow_sweep_nodes(const BowNodes &c, int lane, int32_t *status)
{
    bool bad = false;
    for (int k = blockIdx.x * 256 + threadIdx.x; k < c.nnodes; k += gridDim.x * 256) {
        const int o0 = c.off[k], o1 = c.off[k + 1];
        bad = bad || (k > 0 && c.nodes[k - 1] >= c.nodes[k]) || o0 < 0 || o1 < o0 || o1 > c.n;
    }
    if (__any(bad) && lane == 0) *status = ORBFE_ERR_INVALID;
}

// The lane's next candidate in list order, at distance d, against its running best (d1 at chunk c1, index i1; d2 the runner-up): the
// if-chain of :213-222.  Written as selects on purpose: as an if / else-if behind these references the compiler branches around the
// update, 2 - 3 % of the kernels' GPU time.
__device__ __forceinline__ void bow_walk_offer(int d, int c, int idx, int &d1, int &d2, int &c1, int &i1)
{
    const bool take = d < d1;
    d2 = take ? d1 : (d < d2 ? d : d2);
    d1 = take ? d : d1; c1 = take ? c : c1; i1 = take ? idx : i1;
}

// The walk of one shared node, by one wave, for both SearchByFboW overloads.  The QUERY side is the outer loop of the reference
// (:203 / :563): its list entries q_list[k0, k1) are taken in list order, those with q_valid set.  The CANDIDATE side is the inner
// loop (:213 / :567): position j of c_list[f0, f0 + nf) belongs to lane j & 63 (its chunk j >> 6).  The flag "candidate already
// matched" of chunk c < BOW_FLAG_CHUNKS is bit c of the lane's `taken`; where the flag of a later chunk lives, which candidates
// count at all, where an accepted pair is written and the bound on bestDist1 are the Side's:
//   BOUND               accept at bestDist1 <= BOUND (:225 `<= TH_LOW`, :593 `< TH_LOW`)
//   usable(idx)         folded in when a candidate is loaded
//   late_reset(idx)     before the first query, for every candidate of a chunk >= BOW_FLAG_CHUNKS, by the lane that owns it
//   late_taken(idx)     the flag of such a candidate; only the lane that owns it reads and writes it
//   accept(q, idx, late)
// A lane's candidates come in list order, so its running (d1, d2) is the if-chain of :213-222 on its share; the wave's bestDist1 is
// the smallest key d << 16 | j (first minimum in list order), bestDist2 the smallest distance of all the others, duplicates of
// bestDist1 included.  Every index is checked before it is used as an address; returns whether this lane refused one.
template <class Side>
__device__ __forceinline__ bool bow_node_walk(const Side &s, float nnratio, const int32_t *q_list, int k0, int k1, const int32_t *q_valid, const uint8_t *q_desc, int n_q,
                                              const int32_t *c_list, int f0, int nf, const uint8_t *c_desc, int n, int lane)
{
    bool bad = false;
    // this lane's first BOW_REG_CHUNKS candidates stay in registers: few nodes hold more than 64 * BOW_REG_CHUNKS
    int idxc[BOW_REG_CHUNKS];
    uint32_t fdc[BOW_REG_CHUNKS][8];
#pragma unroll
    for (int c = 0; c < BOW_REG_CHUNKS; c++) {
        const int j = lane + 64 * c;
        idxc[c] = j < nf ? c_list[f0 + j] : -1;
        if (j < nf && (idxc[c] < 0 || idxc[c] >= n)) { bad = true; idxc[c] = -1; }
        // the descriptor of every entry inside the array, before the Side's verdict: its loads run beside the Side's, not behind them
#pragma unroll
        for (int k = 0; k < 8; k++) fdc[c][k] = idxc[c] >= 0 ? ((const uint32_t *)(c_desc + (size_t)idxc[c] * 32))[k] : 0u;
        if (idxc[c] >= 0 && !s.usable(idxc[c])) idxc[c] = -1;
    }
    // the rest of the list is read in place by every query: its indices are checked, and its late flags zeroed, once
    for (int j = lane + 64 * BOW_REG_CHUNKS; j < nf; j += 64) {
        const int idx = c_list[f0 + j];
        const bool out = idx < 0 || idx >= n;
        bad = bad || out;
        if (j >= 64 * BOW_FLAG_CHUNKS && !out) s.late_reset(idx);
    }
    u64 taken = 0;
    for (int kbase = k0; kbase < k1; kbase += 64) {
        // 64 queries at a time are fetched by the lanes side by side, so that no load sits in the sequential loop below
        int my_kf = -1;
        bool my_ok = false;
        uint32_t my_kd[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (kbase + lane < k1) {
            my_kf = q_list[kbase + lane];
            if (my_kf < 0 || my_kf >= n_q) bad = true;
            else if (q_valid[my_kf]) {
                my_ok = true;
#pragma unroll
                for (int k = 0; k < 8; k++) my_kd[k] = ((const uint32_t *)(q_desc + (size_t)my_kf * 32))[k];
            }
        }
        for (u64 todo = __ballot(my_ok); todo; todo &= todo - 1) { // the valid queries in order
            const int src = __ffsll((long long)todo) - 1;
            const int real_kf = __builtin_amdgcn_readlane(my_kf, src);
            uint32_t kd[8];
#pragma unroll
            for (int k = 0; k < 8; k++) kd[k] = (uint32_t)__builtin_amdgcn_readlane((int)my_kd[k], src);
            int d1 = 256, d2 = 256, c1 = 1023, i1 = -1; // 256 differing bits are no candidate (`dist < bestDist1`), chunk 1023 is none
#pragma unroll
            for (int c = 0; c < BOW_REG_CHUNKS; c++) {
                if (idxc[c] < 0 || ((taken >> c) & 1ull)) continue;
                bow_walk_offer(hamming256(kd, fdc[c]), c, idxc[c], d1, d2, c1, i1);
            }
            for (int j = lane + 64 * BOW_REG_CHUNKS, c = BOW_REG_CHUNKS; j < nf; j += 64, c++) {
                const int idx = c_list[f0 + j];
                if (idx < 0 || idx >= n) continue;
                if (!s.usable(idx)) continue;
                if (c < BOW_FLAG_CHUNKS ? (int)((taken >> c) & 1ull) : (int)s.late_taken(idx)) continue;
                bow_walk_offer(hamming256(kd, (const uint32_t *)(c_desc + (size_t)idx * 32)), c, idx, d1, d2, c1, i1);
            }
            // bestDist1: the smallest key distance << 16 | list position (chunk * 64 + lane): the first minimum in list order
            const unsigned key = ((unsigned)d1 << 16) | (unsigned)(c1 * 64 + lane);
            const unsigned m = wave_min_u32_dpp(key);
            const int best1 = (int)(m >> 16);
            if (best1 > Side::BOUND) continue; // also: no candidate at all
            const bool winner = key == m; // list positions are unique
            const int best2 = (int)wave_min_u32_dpp((unsigned)(winner ? d2 : d1)); // the smallest of all the others, duplicates of bestDist1 included
            if (!((float)best1 < nnratio * (float)best2)) continue;
            if (winner) {
                s.accept(real_kf, i1, c1 >= BOW_FLAG_CHUNKS);
                if (c1 < BOW_FLAG_CHUNKS) taken |= 1ull << c1;
            }
        }
    }
    return bad;
}

// SearchByFboW(KeyFrame*, Frame&): the keyframe's features are the queries, every frame keypoint of the node is a candidate, the
// result is indexed by the candidate (f_match[idxF] = realIdxKF, :227), so the flag of a late chunk is f_match itself, which only
// the lane that owns the keypoint wrote (every frame keypoint lies in one node).
struct BowFrameSide {
    static constexpr int BOUND = TH_LOW;
    int32_t *match;
    __device__ __forceinline__ bool usable(int) const { return true; }
    __device__ __forceinline__ void late_reset(int) const {}
    __device__ __forceinline__ bool late_taken(int idx) const { return match[idx] >= 0; }
    __device__ __forceinline__ void accept(int q, int idx, bool) const { match[idx] = q; }
};

// One wave per keyframe node.  The frame's node count is the device's own, clamped to the capacity, which also bounds its CSR.
// RECORD: `a` was built from a record in memory (bow_batch_row).  Then the loads of the keyframe's node are flat loads, and that of
// *f_n_nodes, left to the compiler, sinks behind the node's checks as one more in the wave's chain (2 % of the batch call's GPU time):
// readfirstlane (the count is wave-uniform) keeps it here, beside the slot's count.  With kernel-argument pointers it stays a scalar
// load that needs no such help, and the wait that readfirstlane brings costs the single call 1 %.
template <bool RECORD>
__device__ __forceinline__ void bow_node_match(const BowSearch &a)
{
    const int lane = threadIdx.x & 63;
    const int node = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (node >= a.kf_nnodes) return;
    const int n = slot_count(a.n_ptr, a.cap);
    if (n == 0) return;
    int nfn = slot_count(a.f_n_nodes, a.cap);
    if (RECORD) nfn = __builtin_amdgcn_readfirstlane(nfn);
    const BowNodes kf = {a.kf_nodes, a.kf_off, a.kf_nnodes, a.n_kf}, f = {a.f_nodes, a.f_off, nfn, a.cap};
    int k0, k1, f0, nf;
    if (!bow_shared_node<RECORD>(kf, f, node, lane, a.status, k0, k1, f0, nf)) return;
    const BowFrameSide side = {a.match};
    const bool bad = bow_node_walk(side, a.nnratio, a.kf_feat, k0, k1, a.kf_valid, a.kf_desc, a.n_kf, a.f_feat, f0, nf, a.desc, n, lane);
    if (__any(bad) && lane == 0) *a.status = ORBFE_ERR_INVALID;
}

// One workgroup.  A frame keypoint is matched at most once, so the accepted events are the non-negative entries of f_match.
__device__ __forceinline__ void bow_match_tail(const BowSearch &a)
{
    __shared__ int32_t s_hist[32];
    __shared__ int s_keep[3], s_nm;
    const int tid = threadIdx.x;
    const int n = slot_count(a.n_ptr, a.cap);
    if (tid < 32) s_hist[tid] = 0;
    if (tid == 0) s_nm = 0;
    __syncthreads();
    if (a.check_ori) {
        for (int k = tid; k < n; k += 1024) {
            const int m = a.match[k];
            if (m < 0) continue;
            int bin = orbfe_resolve::rot_bin(a.kf_angle[m], a.keys[k].angle); // rotHist[bin].push_back(bestIdxF), :240-250
            if ((unsigned)bin >= (unsigned)HISTO_LENGTH) { bin = 0; *a.status = ORBFE_ERR_INVALID; } // angles outside [0, 360)
            atomicAdd(&s_hist[bin], 1);
        }
        __syncthreads();
        if (tid == 0) orbfe_resolve::three_maxima(s_hist, HISTO_LENGTH, &s_keep[0], &s_keep[1], &s_keep[2]);
        __syncthreads();
    }
    int cnt = 0;
    for (int k = tid; k < n; k += 1024) {
        int m = a.match[k];
        if (m >= 0 && a.check_ori) {
            int bin = orbfe_resolve::rot_bin(a.kf_angle[m], a.keys[k].angle);
            if ((unsigned)bin >= (unsigned)HISTO_LENGTH) bin = 0;
            if (bin != s_keep[0] && bin != s_keep[1] && bin != s_keep[2]) { a.match[k] = -1; m = -1; } // :263-278
        }
        cnt += m >= 0;
        if (a.has_point) a.has_point[k] = m >= 0;
        if (a.Xw && a.kf_pos && m >= 0) {
            a.Xw[3 * k] = a.kf_pos[3 * m];
            a.Xw[3 * k + 1] = a.kf_pos[3 * m + 1];
            a.Xw[3 * k + 2] = a.kf_pos[3 * m + 2];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((tid & 63) == 0 && cnt) atomicAdd(&s_nm, cnt);
    __syncthreads();
    if (tid == 0) *a.nmatches = s_nm;
}

__global__ __launch_bounds__(256) void bow_match_init_kernel(BowSearch a) { bow_match_init(a); }
__global__ __launch_bounds__(256) void bow_node_match_kernel(BowSearch a) { bow_node_match<false>(a); }
__global__ __launch_bounds__(1024) void bow_match_tail_kernel(BowSearch a) { bow_match_tail(a); }

// The batch: `a` holds the frame's side, the settings and row 0 of the outputs.  Record k is the same for every lane (k is a
// workgroup index) and is read before any store, so it arrives by scalar loads and the BowSearch built from it stays in SGPRs.
// A record the single call would refuse on the host (a negative count, a NULL array under nnodes > 0), or whose nnodes lies
// outside [0, max_kf_nnodes] (the node grid would not cover it), is searched as a keyframe without nodes and reported in its status.
static_assert(sizeof(orbfe_bow_keyframe) == 64, "orbfe_bow_keyframe: seven pointers and two counts");
__device__ __forceinline__ BowSearch bow_batch_row(BowSearch a, const orbfe_bow_keyframe *__restrict__ kfs, int max_kf_nnodes, int k, bool *refused)
{
    const orbfe_bow_keyframe kf = kfs[k];
    *refused = kf.nnodes < 0 || kf.nnodes > max_kf_nnodes || kf.n < 0 ||
               (kf.nnodes > 0 && (!kf.nodes || !kf.off || !kf.feat || !kf.valid || !kf.desc || !kf.angle));
    a.kf_nodes = kf.nodes; a.kf_off = kf.off; a.kf_feat = kf.feat; a.kf_nnodes = *refused ? 0 : kf.nnodes;
    a.kf_valid = kf.valid; a.kf_desc = kf.desc; a.kf_angle = kf.angle; a.n_kf = kf.n; a.kf_pos = kf.pos;
    a.match += (size_t)k * a.cap; a.nmatches += k; a.status += k;
    if (a.has_point) a.has_point += (size_t)k * a.cap;
    if (a.Xw) a.Xw += (size_t)k * a.cap * 3;
    return a;
}

__global__ __launch_bounds__(256) void bow_match_init_batch_kernel(BowSearch a, const orbfe_bow_keyframe *__restrict__ kfs, int max_kf_nnodes)
{
    bool refused;
    const BowSearch r = bow_batch_row(a, kfs, max_kf_nnodes, blockIdx.y, &refused);
    bow_match_init(r);
    if (refused && blockIdx.x == 0 && threadIdx.x == 0) *r.status = ORBFE_ERR_INVALID; // the thread that wrote it in bow_match_init
}
__global__ __launch_bounds__(256) void bow_node_match_batch_kernel(BowSearch a, const orbfe_bow_keyframe *__restrict__ kfs, int max_kf_nnodes)
{
    bool refused;
    bow_node_match<true>(bow_batch_row(a, kfs, max_kf_nnodes, blockIdx.y, &refused)); // a node at or past kf_nnodes returns first of all
}
__global__ __launch_bounds__(1024) void bow_match_tail_batch_kernel(BowSearch a, const orbfe_bow_keyframe *__restrict__ kfs, int max_kf_nnodes)
{
    bool refused;
    bow_match_tail(bow_batch_row(a, kfs, max_kf_nnodes, blockIdx.x, &refused));
}

// The slot's side of a BowSearch and the checks both entry points share.
static int bow_search_frame_side(orbfe_context *ctx, int slot, BowSearch *a)
{
    const DeviceConfig *cfg = &ctx->cfg;
    const DeviceBuffers *buf = &ctx->buf;
    if (slot < 0 || slot >= ctx->last_images)
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "device slot %d: the latest extraction call filled %d image slots", slot, ctx->last_images);
    const int cap = cfg->sel_total;
    if (cap <= 0 || cap > 65535) return orbfe_fail(ctx, ORBFE_ERR_UNSUPPORTED, "frames with more than 65535 keypoints are not supported");
    a->keys = (const KeyPointPOD *)buf->kps + (size_t)slot * cap; // mvKeys[].angle
    a->desc = buf->desc + (size_t)slot * cap * 32;
    a->n_ptr = buf->kp_cnt + slot; a->cap = cap;
    return ORBFE_OK;
}

extern "C" int orbfe_enqueue_search_by_bow(orbfe_context *ctx, int slot,
                                           const uint32_t *d_kf_nodes, const int32_t *d_kf_off, const int32_t *d_kf_feat, int kf_nnodes,
                                           const int32_t *d_kf_valid, const uint8_t *d_kf_desc, const float *d_kf_angle, int n_kf, const float *d_kf_pos,
                                           const uint32_t *d_f_nodes, const int32_t *d_f_off, const int32_t *d_f_feat, const int32_t *d_f_n_nodes,
                                           float nnratio, int check_ori, int32_t *d_f_match, int32_t *d_nmatches, int32_t *d_status,
                                           uint8_t *d_has_point, float *d_Xw, void *stream)
try {
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    ORBFE_ENTRY(ctx);
    if (kf_nnodes < 0 || n_kf < 0 || !d_f_nodes || !d_f_off || !d_f_feat || !d_f_n_nodes || !d_f_match || !d_nmatches || !d_status ||
        (kf_nnodes > 0 && (!d_kf_nodes || !d_kf_off || !d_kf_feat || !d_kf_valid || !d_kf_desc || !d_kf_angle)))
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null argument");
    BowSearch a;
    int rc = bow_search_frame_side(ctx, slot, &a);
    if (rc != ORBFE_OK) return rc;
    const int cap = a.cap;
    hipStream_t s;
    rc = orbfe_enqueue_on(ctx, stream, true, &s);
    if (rc != ORBFE_OK) return rc;
    a.kf_nodes = d_kf_nodes; a.kf_off = d_kf_off; a.kf_feat = d_kf_feat; a.kf_nnodes = kf_nnodes;
    a.kf_valid = d_kf_valid; a.kf_desc = d_kf_desc; a.kf_angle = d_kf_angle; a.n_kf = n_kf; a.kf_pos = d_kf_pos;
    a.f_nodes = d_f_nodes; a.f_off = d_f_off; a.f_feat = d_f_feat; a.f_n_nodes = d_f_n_nodes;
    a.nnratio = nnratio; a.check_ori = check_ori != 0;
    a.match = d_f_match; a.nmatches = d_nmatches; a.status = d_status; a.has_point = d_has_point; a.Xw = d_Xw;
    hipLaunchKernelGGL(bow_match_init_kernel, dim3((cap + 255) / 256), dim3(256), 0, s, a);
    if (kf_nnodes > 0) hipLaunchKernelGGL(bow_node_match_kernel, dim3((kf_nnodes + 3) / 4), dim3(256), 0, s, a);
    hipLaunchKernelGGL(bow_match_tail_kernel, dim3(1), dim3(1024), 0, s, a);
    ORBFE_HIP_TRY(ctx, hipGetLastError());
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

extern "C" int orbfe_enqueue_search_by_bow_batch(orbfe_context *ctx, int slot, const orbfe_bow_keyframe *d_kfs, int n_kfs, int max_kf_nnodes,
                                                 const uint32_t *d_f_nodes, const int32_t *d_f_off, const int32_t *d_f_feat, const int32_t *d_f_n_nodes,
                                                 float nnratio, int check_ori, int32_t *d_f_match, int32_t *d_nmatches, int32_t *d_status,
                                                 uint8_t *d_has_point, float *d_Xw, void *stream)
try {
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    ORBFE_ENTRY(ctx);
    if (n_kfs < 0 || n_kfs > 65535 || max_kf_nnodes < 0)
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "n_kfs = %d (0 .. 65535, the grid's y limit), max_kf_nnodes = %d", n_kfs, max_kf_nnodes);
    if (!d_f_nodes || !d_f_off || !d_f_feat || !d_f_n_nodes || !d_f_match || !d_nmatches || !d_status || (n_kfs > 0 && !d_kfs))
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null argument");
    BowSearch a;
    int rc = bow_search_frame_side(ctx, slot, &a);
    if (rc != ORBFE_OK) return rc;
    if (n_kfs == 0) return ORBFE_OK;
    const int cap = a.cap;
    hipStream_t s;
    rc = orbfe_enqueue_on(ctx, stream, true, &s);
    if (rc != ORBFE_OK) return rc;
    a.kf_nodes = nullptr; a.kf_off = a.kf_feat = a.kf_valid = nullptr; a.kf_desc = nullptr; a.kf_angle = a.kf_pos = nullptr; // per record, on the device
    a.kf_nnodes = a.n_kf = 0;
    a.f_nodes = d_f_nodes; a.f_off = d_f_off; a.f_feat = d_f_feat; a.f_n_nodes = d_f_n_nodes;
    a.nnratio = nnratio; a.check_ori = check_ori != 0;
    a.match = d_f_match; a.nmatches = d_nmatches; a.status = d_status; a.has_point = d_has_point; a.Xw = d_Xw; // row 0
    hipLaunchKernelGGL(bow_match_init_batch_kernel, dim3((cap + 255) / 256, n_kfs), dim3(256), 0, s, a, d_kfs, max_kf_nnodes);
    if (max_kf_nnodes > 0) hipLaunchKernelGGL(bow_node_match_batch_kernel, dim3((max_kf_nnodes + 3) / 4, n_kfs), dim3(256), 0, s, a, d_kfs, max_kf_nnodes);
    hipLaunchKernelGGL(bow_match_tail_batch_kernel, dim3(n_kfs), dim3(1024), 0, s, a, d_kfs, max_kf_nnodes);
    ORBFE_HIP_TRY(ctx, hipGetLastError());
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

// ---------------------------------------------------------------------------------------------
// SearchForTriangulation(KeyFrame*, KeyFrame*) (src/ORBmatcher.cc:652-819)
// ---------------------------------------------------------------------------------------------
static_assert(sizeof(orbfe_tri_keyframe) == 64, "orbfe_tri_keyframe: seven pointers and two counts");
static_assert(sizeof(orbfe_keypoint) == sizeof(KeyPointPOD), "orbfe_keypoint is the extraction's keypoint record");

struct TriSearch {
    orbfe_tri_keyframe k1, k2;
    float F12[9], ex, ey;                                         // the three small matrices travel as kernel arguments; the epipole is the host's
    float scale[ORBFE_MAX_LEVELS], sigma2[ORBFE_MAX_LEVELS];      // mvScaleFactors, mvLevelSigma2
    int nlevels, only_stereo, check_ori;
    int32_t *match12, *pairs, *nmatches, *status;
    uint8_t *taken2;                                              // [k2.n] scratch: vbMatched2 beyond the lane-held flags; NULL when no node can reach that far
};

__global__ __launch_bounds__(256) void tri_init_kernel(TriSearch a)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k == 0) { *a.status = ORBFE_OK; *a.nmatches = 0; }
    if (k < a.k1.n) a.match12[k] = -1;
}

// What a lane knows of one KF2 feature of the node: idx < 0 is no candidate (beyond the list, refused, has a map point, monocular
// under only_stereo).
struct TriCand {
    int idx;
    uint32_t d[8];
    float x, y, scale, sigma2;
    bool stereo;
};

// Feature `j` of the node's KF2 list.  Every index is checked before it is used as an address; `bad` collects what is refused.
__device__ __forceinline__ void tri_load_cand(const TriSearch &a, int f0, int nf, int j, TriCand &c, bool &bad)
{
    c.idx = -1; c.x = c.y = 0.f; c.scale = c.sigma2 = 1.f; c.stereo = false;
#pragma unroll
    for (int k = 0; k < 8; k++) c.d[k] = 0u;
    if (j >= nf) return;
    const int idx = a.k2.feat[f0 + j];
    if (idx < 0 || idx >= a.k2.n) { bad = true; return; }
    if (a.k2.has_mp[idx]) return;
    const bool stereo = a.k2.u_right[idx] >= 0;
    if (a.only_stereo && !stereo) return;
    const orbfe_keypoint *kp = a.k2.keys_un + idx;
    const int octave = kp->octave;
    if (octave < 0 || octave >= a.nlevels) { bad = true; return; }
    c.idx = idx; c.stereo = stereo; c.x = kp->x; c.y = kp->y; c.scale = a.scale[octave]; c.sigma2 = a.sigma2[octave];
#pragma unroll
    for (int k = 0; k < 8; k++) c.d[k] = ((const uint32_t *)(a.k2.desc + (size_t)idx * 32))[k];
}

// One wave per KF1 node: the sweep and the merge-join step of the SearchByFboW kernels, then a loop of its own (on bow_node_walk the
// 20 enqueues of tools/bench_matchers.py --triangulation took 1.3 - 2 % more GPU time than this loop, and neither the resource table
// nor the disassembly said why: DESIGN.md §4f).  A KF2 keypoint lies in one node of KF2's feature vector, so vbMatched2 (:719, :756)
// is read and written only by the KF1 features of the same node: the rule is sequential inside a node and nowhere else.  The wave
// takes the node's usable KF1 features in list order; position j of the node's KF2 list belongs to lane j & 63 (chunk j >> 6).  The
// flag "KF2 keypoint taken" of chunk c < BOW_FLAG_CHUNKS is bit c of the lane's `taken`, of a later chunk it is taken2[idx2], which
// this lane zeroes before the first query and which only it touches.  The reference's inner loop (:712-750) keeps the LAST candidate
// of the smallest distance that passes every gate (`dist > bestDist` skips, bestDist starts at TH_LOW, and bestDist only moves when
// CheckDistEpipolarLine accepts): a lane's candidates come in list order, so `d <= d1` keeps its last minimum, and the wave's winner
// is the smallest key d << 16 | (0xffff - position).  No ratio test.
__global__ __launch_bounds__(256) void tri_node_match_kernel(TriSearch a)
{
    const int lane = threadIdx.x & 63;
    const int n1 = a.k1.n;
    const BowNodes kf1 = {a.k1.nodes, a.k1.off, a.k1.nnodes, n1}, kf2 = {a.k2.nodes, a.k2.off, a.k2.nnodes, a.k2.n};
    bow_sweep_nodes(kf2, lane, a.status);
    int k0, k1, f0, nf;
    if (!bow_shared_node<false>(kf1, kf2, blockIdx.x * 4 + (threadIdx.x >> 6), lane, a.status, k0, k1, f0, nf)) return;
    bool bad = false;
    for (int j = lane + 64 * BOW_FLAG_CHUNKS; j < nf; j += 64) { // the late flags of this lane's positions (nf > 4096: taken2 is not NULL)
        const int idx = a.k2.feat[f0 + j];
        if (idx >= 0 && idx < a.k2.n) a.taken2[idx] = 0;
    }
    TriCand rc[BOW_REG_CHUNKS];
#pragma unroll
    for (int c = 0; c < BOW_REG_CHUNKS; c++) tri_load_cand(a, f0, nf, lane + 64 * c, rc[c], bad);
    u64 taken = 0;
    for (int kbase = k0; kbase < k1; kbase += 64) {
        // 64 KF1 features at a time are fetched by the lanes side by side, so that no load of KF1 sits in the sequential loop below
        int my_i1 = -1;
        bool my_ok = false, my_stereo = false;
        float my_x = 0.f, my_y = 0.f;
        uint32_t my_d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (kbase + lane < k1) {
            my_i1 = a.k1.feat[kbase + lane];
            if (my_i1 < 0 || my_i1 >= n1) bad = true;
            else if (!a.k1.has_mp[my_i1]) {
                my_stereo = a.k1.u_right[my_i1] >= 0;
                if (!a.only_stereo || my_stereo) {
                    my_ok = true;
                    my_x = a.k1.keys_un[my_i1].x; my_y = a.k1.keys_un[my_i1].y;
#pragma unroll
                    for (int k = 0; k < 8; k++) my_d[k] = ((const uint32_t *)(a.k1.desc + (size_t)my_i1 * 32))[k];
                }
            }
        }
        const u64 stereo_mask = __ballot(my_stereo);
        for (u64 todo = __ballot(my_ok); todo; todo &= todo - 1) { // the usable KF1 features in list order
            const int src = __ffsll((long long)todo) - 1;
            const int idx1 = __builtin_amdgcn_readlane(my_i1, src);
            const float x1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_x), src));
            const float y1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_y), src));
            const bool stereo1 = (stereo_mask >> src) & 1ull;
            uint32_t kd[8];
#pragma unroll
            for (int k = 0; k < 8; k++) kd[k] = (uint32_t)__builtin_amdgcn_readlane((int)my_d[k], src);
            int d1 = 256, c1 = 0, i2 = -1; // 256 differing bits: no candidate yet
#pragma unroll
            for (int c = 0; c < BOW_REG_CHUNKS; c++) {
                const TriCand &q = rc[c];
                if (q.idx < 0 || ((taken >> c) & 1ull)) continue;
                const int d = hamming256(kd, q.d);
                if (d > TH_LOW || d > d1) continue;
                if (!stereo1 && !q.stereo && orbfe_epipolar::inside_epipole_disc(a.ex, a.ey, q.x, q.y, q.scale)) continue;
                if (!orbfe_epipolar::check_dist_epipolar_line(x1, y1, q.x, q.y, a.F12, q.sigma2)) continue;
                d1 = d; c1 = c; i2 = q.idx;
            }
            for (int j = lane + 64 * BOW_REG_CHUNKS, c = BOW_REG_CHUNKS; j < nf; j += 64, c++) { // nodes beyond 64 * BOW_REG_CHUNKS features: read in place
                TriCand q;
                tri_load_cand(a, f0, nf, j, q, bad);
                if (q.idx < 0) continue;
                if (c < BOW_FLAG_CHUNKS ? (int)((taken >> c) & 1ull) : (int)a.taken2[q.idx]) continue;
                const int d = hamming256(kd, q.d);
                if (d > TH_LOW || d > d1) continue;
                if (!stereo1 && !q.stereo && orbfe_epipolar::inside_epipole_disc(a.ex, a.ey, q.x, q.y, q.scale)) continue;
                if (!orbfe_epipolar::check_dist_epipolar_line(x1, y1, q.x, q.y, a.F12, q.sigma2)) continue;
                d1 = d; c1 = c; i2 = q.idx;
            }
            // the smallest distance; among equals the largest list position (chunk * 64 + lane < 65535): the last one the reference's loop meets
            const unsigned key = ((unsigned)d1 << 16) | (0xffffu - (unsigned)(c1 * 64 + lane));
            const unsigned m = wave_min_u32_dpp(key);
            if ((int)(m >> 16) > TH_LOW) continue; // no candidate at all
            if (key == m) { // list positions are unique
                a.match12[idx1] = i2;
                if (c1 < BOW_FLAG_CHUNKS) taken |= 1ull << c1;
                else a.taken2[i2] = 1;
            }
        }
    }
    if (__any(bad) && lane == 0) *a.status = ORBFE_ERR_INVALID;
}

// One workgroup of 1024, for the matchers whose result is match12[idx1] = idx2.  A KF1 keypoint lies in one node, so the accepted
// pairs are the non-negative entries of match12 (each a KF2 index the node kernel checked): rotation histogram (:781-790, :602-609;
// the bin collects idx1), ComputeThreeMaxima, losers removed (:793-806, :619-633), the count, and the accepted (idx1, idx2) in
// ascending idx1 (vMatchedPairs, :808-816; the order in which Sim3Solver walks vpMatched12) by an ordered compaction: thread t owns
// a contiguous run of idx1, the runs' counts are scanned.  At most `room` pairs are written.
template <class Angle1, class Angle2>
__device__ __forceinline__ void match12_tail(int n1, int32_t *match12, int32_t *pairs, int room, int32_t *nmatches, int32_t *status, int check_ori,
                                             Angle1 angle1, Angle2 angle2)
{
    __shared__ int32_t s_hist[32];
    __shared__ int s_keep[3], s_wave[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 32) s_hist[tid] = 0;
    __syncthreads();
    if (check_ori) {
        for (int k = tid; k < n1; k += 1024) {
            const int m = match12[k];
            if (m < 0) continue;
            int bin = orbfe_resolve::rot_bin(angle1(k), angle2(m)); // rotHist[bin].push_back(idx1)
            if ((unsigned)bin >= (unsigned)HISTO_LENGTH) { bin = 0; *status = ORBFE_ERR_INVALID; } // angles outside [0, 360)
            atomicAdd(&s_hist[bin], 1);
        }
        __syncthreads();
        if (tid == 0) orbfe_resolve::three_maxima(s_hist, HISTO_LENGTH, &s_keep[0], &s_keep[1], &s_keep[2]);
        __syncthreads();
    }
    const int run = (n1 + 1023) / 1024;
    const int lo = tid * run < n1 ? tid * run : n1, hi = lo + run < n1 ? lo + run : n1;
    int cnt = 0;
    for (int k = lo; k < hi; k++) {
        int m = match12[k];
        if (m >= 0 && check_ori) {
            int bin = orbfe_resolve::rot_bin(angle1(k), angle2(m));
            if ((unsigned)bin >= (unsigned)HISTO_LENGTH) bin = 0;
            if (bin != s_keep[0] && bin != s_keep[1] && bin != s_keep[2]) { match12[k] = -1; m = -1; }
        }
        cnt += m >= 0;
    }
    int incl = cnt; // inclusive scan inside the wave, then over the 16 wave totals
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < 16; w++) {
        const int t = s_wave[w];
        before += w < wave ? t : 0;
        total += t;
    }
    if (tid == 0) *nmatches = total;
    if (!pairs) return;
    int p = before + incl - cnt;
    for (int k = lo; k < hi && p < room; k++) {
        const int m = match12[k];
        if (m < 0) continue;
        pairs[2 * p] = k; pairs[2 * p + 1] = m;
        p++;
    }
}

__global__ __launch_bounds__(1024) void tri_tail_kernel(TriSearch a)
{
    // a KF2 keypoint is taken once, so the count <= min(n1, n2), the caller's array; only a refused feature vector (a KF2 keypoint in
    // two nodes) can exceed it, and then the rest is dropped
    match12_tail(a.k1.n, a.match12, a.pairs, a.k1.n < a.k2.n ? a.k1.n : a.k2.n, a.nmatches, a.status, a.check_ori,
                 [&](int k) { return a.k1.keys_un[k].angle; }, [&](int m) { return a.k2.keys_un[m].angle; });
}

extern "C" int orbfe_enqueue_search_for_triangulation(orbfe_context *ctx, const orbfe_tri_keyframe *kf1, const orbfe_tri_keyframe *kf2,
                                                      const float *F12, const float *Cw1, const float *T2w, float fx2, float fy2, float cx2, float cy2,
                                                      int only_stereo, int check_ori, int32_t *d_match12, int32_t *d_pairs, int32_t *d_nmatches,
                                                      int32_t *d_status, void *stream)
try {
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    ORBFE_ENTRY(ctx);
    if (!kf1 || !kf2 || !F12 || !Cw1 || !T2w || !d_match12 || !d_nmatches || !d_status) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null argument");
    for (const orbfe_tri_keyframe *kf : {kf1, kf2}) {
        if (kf->n < 0 || kf->nnodes < 0) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "negative count");
        if (kf->n > 65535) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "keyframes with more than 65535 keypoints are not supported");
        if (kf->nnodes > 0 && (!kf->nodes || !kf->off || !kf->feat || !kf->keys_un || !kf->u_right || !kf->has_mp || !kf->desc))
            return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null array in a keyframe record with nodes");
    }
    const int nlevels = ctx->params.nlevels;
    if (nlevels < 1 || nlevels > ORBFE_MAX_LEVELS) return orbfe_fail(ctx, ORBFE_ERR_UNSUPPORTED, "nlevels = %d", nlevels);
    hipStream_t s;
    if (const int rc = orbfe_enqueue_on(ctx, stream, false, &s)) return rc;
    TriSearch a;
    a.taken2 = nullptr;
    if (kf2->n > 64 * BOW_FLAG_CHUNKS) { // as bowkf_fill: below that no node list reaches a position whose flag needs memory
        orbfe_bow_state *st = orbfe_ctx_bow_state(ctx);
        if (!st) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "out of host memory");
        if (st->resident.ensure((size_t)kf2->n)) return orbfe_fail(ctx, ORBFE_ERR_HIP, "BoW scratch allocation failed");
        a.taken2 = (uint8_t *)st->resident.p;
    }
    a.k1 = *kf1; a.k2 = *kf2; // a record without nodes may hold NULL arrays: the tail follows keys_un only through a match
    for (int k = 0; k < 9; k++) a.F12[k] = F12[k];
    orbfe_epipolar::epipole(Cw1, T2w, fx2, fy2, cx2, cy2, &a.ex, &a.ey);
    const float *scale = ctx->plan.scale;
    for (int l = 0; l < ORBFE_MAX_LEVELS; l++) {
        a.scale[l] = l < nlevels ? scale[l] : 1.f;
        a.sigma2[l] = a.scale[l] * a.scale[l]; // mvLevelSigma2 (src/ORBextractor.cc:419-423)
    }
    a.nlevels = nlevels; a.only_stereo = only_stereo != 0; a.check_ori = check_ori != 0;
    a.match12 = d_match12; a.pairs = d_pairs; a.nmatches = d_nmatches; a.status = d_status;
    hipLaunchKernelGGL(tri_init_kernel, dim3(a.k1.n > 0 ? (a.k1.n + 255) / 256 : 1), dim3(256), 0, s, a);
    if (a.k1.nnodes > 0 && a.k2.nnodes > 0) hipLaunchKernelGGL(tri_node_match_kernel, dim3((a.k1.nnodes + 3) / 4), dim3(256), 0, s, a);
    hipLaunchKernelGGL(tri_tail_kernel, dim3(1), dim3(1024), 0, s, a);
    ORBFE_HIP_TRY(ctx, hipGetLastError());
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

// ---------------------------------------------------------------------------------------------
// SearchByFboW(KeyFrame*, KeyFrame*) (src/ORBmatcher.cc:517-650), LoopClosing::ComputeSim3 (src/LoopClosing.cc:288-316)
// ---------------------------------------------------------------------------------------------
// Both keyframes are orbfe_bow_keyframe records of device pointers.  vbMatched2[idx2] (:571 read, :598 written) is touched only by
// the KF1 features of the node that holds idx2, so the rule is sequential inside a node and nowhere else: bow_node_walk with KF1 as
// the query side.  Three launches whatever the number of candidates (the candidates of ComputeSim3 are independent: each has its own
// vvpMapPointMatches[i], mpCurrentKF is not written, vbMatched2 is local to one call):
//   bowkf_init_kernel         rows of match12 = -1, count, status
//   bowkf_node_match_kernel   grid (ceil(kf1.nnodes / 4), K), one wave per (KF1 node, candidate)
//   bowkf_tail_kernel         K workgroups: match12_tail
// The _batch kernels run the same device functions on the BowKfSearch that bowkf_batch_row builds from record blockIdx.y (tail:
// blockIdx.x) and that row of the outputs.
struct BowKfSearch {
    orbfe_bow_keyframe k1, k2;                    // pos is never read
    float nnratio; int check_ori;
    int32_t *match12, *pairs, *nmatches, *status;
    uint8_t *taken2;                              // [max n2] scratch: vbMatched2 beyond the lane-held flags; NULL when no node can reach that far
};

// KF1's features are the queries; a KF2 keypoint is a candidate when it has a good map point (valid2, :571-575); the flag sits on the
// candidate (vbMatched2) while the result is indexed by the query (vpMatches12[idx1], :597), so the flag of a late chunk needs memory
// of its own: taken2[idx2], zeroed by the lane that owns position j of the node's list before the first query and touched by no
// other thread (a KF2 keypoint lies in one node).  The bound is strict: bestDist1 < TH_LOW (:593).
struct BowKfSide {
    static constexpr int BOUND = TH_LOW - 1;
    const int32_t *valid2; int32_t *match12; uint8_t *taken2;
    __device__ __forceinline__ bool usable(int idx) const { return valid2[idx] != 0; }
    __device__ __forceinline__ void late_reset(int idx) const { taken2[idx] = 0; }
    __device__ __forceinline__ bool late_taken(int idx) const { return taken2[idx] != 0; }
    __device__ __forceinline__ void accept(int q, int idx, bool late) const
    {
        match12[q] = idx;
        if (late) taken2[idx] = 1;
    }
};

__device__ __forceinline__ void bowkf_init(const BowKfSearch &a, bool refused)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k == 0) { *a.status = refused ? ORBFE_ERR_INVALID : ORBFE_OK; *a.nmatches = 0; }
    if (k < a.k1.n) a.match12[k] = -1;
}

__device__ __forceinline__ void bowkf_node_match(const BowKfSearch &a)
{
    const int lane = threadIdx.x & 63;
    if (a.k2.nnodes == 0) return; // the whole workgroup: a candidate without nodes, or a refused record
    const BowNodes kf1 = {a.k1.nodes, a.k1.off, a.k1.nnodes, a.k1.n}, kf2 = {a.k2.nodes, a.k2.off, a.k2.nnodes, a.k2.n};
    bow_sweep_nodes(kf2, lane, a.status);
    int k0, k1, f0, nf;
    if (!bow_shared_node<false>(kf1, kf2, blockIdx.x * 4 + (threadIdx.x >> 6), lane, a.status, k0, k1, f0, nf)) return;
    const BowKfSide side = {a.k2.valid, a.match12, a.taken2};
    const bool bad = bow_node_walk(side, a.nnratio, a.k1.feat, k0, k1, a.k1.valid, a.k1.desc, a.k1.n, a.k2.feat, f0, nf, a.k2.desc, a.k2.n, lane);
    if (__any(bad) && lane == 0) *a.status = ORBFE_ERR_INVALID;
}

__device__ __forceinline__ void bowkf_tail(const BowKfSearch &a)
{
    // a KF1 keypoint is matched at most once: the count <= n1, the row of d_pairs
    match12_tail(a.k1.n, a.match12, a.pairs, a.k1.n, a.nmatches, a.status, a.check_ori,
                 [&](int k) { return a.k1.angle[k]; }, [&](int m) { return a.k2.angle[m]; });
}

// The batch: `a` holds KF1, the settings and row 0 of the outputs.  Record k is the same for every lane (k is a workgroup index) and
// is read before any store, so it arrives by scalar loads and the BowKfSearch built from it stays in SGPRs.  A record the single
// call would refuse on the host (a negative count, a NULL array under nnodes > 0), or whose n exceeds max_kf_n (the row stride of
// the flags), is searched as a keyframe without nodes and reported in its status.
__device__ __forceinline__ BowKfSearch bowkf_batch_row(BowKfSearch a, const orbfe_bow_keyframe *__restrict__ kfs, int max_kf_n, int k, bool *refused)
{
    const orbfe_bow_keyframe kf = kfs[k];
    *refused = kf.nnodes < 0 || kf.n < 0 || kf.n > max_kf_n ||
               (kf.nnodes > 0 && (!kf.nodes || !kf.off || !kf.feat || !kf.valid || !kf.desc || !kf.angle));
    a.k2 = kf;
    if (*refused) a.k2.nnodes = 0;
    a.match12 += (size_t)k * a.k1.n; a.nmatches += k; a.status += k;
    if (a.pairs) a.pairs += (size_t)k * 2 * a.k1.n;
    if (a.taken2) a.taken2 += (size_t)k * max_kf_n;
    return a;
}

__global__ __launch_bounds__(256) void bowkf_init_kernel(BowKfSearch a) { bowkf_init(a, false); }
__global__ __launch_bounds__(256) void bowkf_node_match_kernel(BowKfSearch a) { bowkf_node_match(a); }
__global__ __launch_bounds__(1024) void bowkf_tail_kernel(BowKfSearch a) { bowkf_tail(a); }
__global__ __launch_bounds__(256) void bowkf_init_batch_kernel(BowKfSearch a, const orbfe_bow_keyframe *__restrict__ kfs, int max_kf_n)
{
    bool refused;
    const BowKfSearch r = bowkf_batch_row(a, kfs, max_kf_n, blockIdx.y, &refused);
    bowkf_init(r, refused);
}
__global__ __launch_bounds__(256) void bowkf_node_match_batch_kernel(BowKfSearch a, const orbfe_bow_keyframe *__restrict__ kfs, int max_kf_n)
{
    bool refused;
    bowkf_node_match(bowkf_batch_row(a, kfs, max_kf_n, blockIdx.y, &refused));
}
__global__ __launch_bounds__(1024) void bowkf_tail_batch_kernel(BowKfSearch a, const orbfe_bow_keyframe *__restrict__ kfs, int max_kf_n)
{
    bool refused;
    bowkf_tail(bowkf_batch_row(a, kfs, max_kf_n, blockIdx.x, &refused));
}

// What the host can see of a record; `what` names it in the message.
static int bowkf_check_record(orbfe_context *ctx, const orbfe_bow_keyframe *kf, const char *what)
{
    if (kf->n < 0 || kf->nnodes < 0) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "%s: negative count", what);
    if (kf->n > 65535) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "%s: keyframes with more than 65535 keypoints are not supported", what);
    if (kf->nnodes > 0 && (!kf->nodes || !kf->off || !kf->feat || !kf->valid || !kf->desc || !kf->angle))
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "%s: null array in a keyframe record with nodes", what);
    return ORBFE_OK;
}

// KF1, the settings, row 0 of the outputs and the flags: n_rows rows of max_n2 bytes of the grow-only BoW scratch, and only when a
// node list can pass the 64 * BOW_FLAG_CHUNKS positions a lane's register covers (a list is no longer than its keyframe's n).
static int bowkf_fill(orbfe_context *ctx, BowKfSearch *a, const orbfe_bow_keyframe *kf1, int n_rows, int max_n2, float nnratio, int check_ori,
                      int32_t *d_match12, int32_t *d_pairs, int32_t *d_nmatches, int32_t *d_status)
{
    a->k1 = *kf1;
    a->nnratio = nnratio; a->check_ori = check_ori != 0;
    a->match12 = d_match12; a->pairs = d_pairs; a->nmatches = d_nmatches; a->status = d_status;
    a->taken2 = nullptr;
    if (max_n2 > 64 * BOW_FLAG_CHUNKS) {
        orbfe_bow_state *st = orbfe_ctx_bow_state(ctx);
        if (!st) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "out of host memory");
        if (st->resident.ensure((size_t)n_rows * (size_t)max_n2)) return orbfe_fail(ctx, ORBFE_ERR_HIP, "BoW scratch allocation failed");
        a->taken2 = (uint8_t *)st->resident.p;
    }
    return ORBFE_OK;
}

extern "C" int orbfe_enqueue_search_by_bow_kf(orbfe_context *ctx, const orbfe_bow_keyframe *kf1, const orbfe_bow_keyframe *kf2, float nnratio, int check_ori,
                                              int32_t *d_match12, int32_t *d_pairs, int32_t *d_nmatches, int32_t *d_status, void *stream)
try {
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    ORBFE_ENTRY(ctx);
    if (!kf1 || !kf2 || !d_match12 || !d_nmatches || !d_status) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null argument");
    int rc = bowkf_check_record(ctx, kf1, "kf1");
    if (rc == ORBFE_OK) rc = bowkf_check_record(ctx, kf2, "kf2");
    if (rc != ORBFE_OK) return rc;
    hipStream_t s;
    rc = orbfe_enqueue_on(ctx, stream, false, &s);
    if (rc != ORBFE_OK) return rc;
    BowKfSearch a;
    rc = bowkf_fill(ctx, &a, kf1, 1, kf2->n, nnratio, check_ori, d_match12, d_pairs, d_nmatches, d_status);
    if (rc != ORBFE_OK) return rc;
    a.k2 = *kf2;
    hipLaunchKernelGGL(bowkf_init_kernel, dim3(a.k1.n > 0 ? (a.k1.n + 255) / 256 : 1), dim3(256), 0, s, a);
    if (a.k1.nnodes > 0 && a.k2.nnodes > 0) hipLaunchKernelGGL(bowkf_node_match_kernel, dim3((a.k1.nnodes + 3) / 4), dim3(256), 0, s, a);
    hipLaunchKernelGGL(bowkf_tail_kernel, dim3(1), dim3(1024), 0, s, a);
    ORBFE_HIP_TRY(ctx, hipGetLastError());
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

extern "C" int orbfe_enqueue_search_by_bow_kf_batch(orbfe_context *ctx, const orbfe_bow_keyframe *kf1, const orbfe_bow_keyframe *d_kfs, int n_kfs, int max_kf_n,
                                                    float nnratio, int check_ori, int32_t *d_match12, int32_t *d_pairs, int32_t *d_nmatches, int32_t *d_status,
                                                    void *stream)
try {
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    ORBFE_ENTRY(ctx);
    if (!kf1 || !d_match12 || !d_nmatches || !d_status || (n_kfs > 0 && !d_kfs)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null argument");
    if (n_kfs < 0 || n_kfs > 65535 || max_kf_n < 0 || max_kf_n > 65535)
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "n_kfs = %d (0 .. 65535, the grid's y limit), max_kf_n = %d (0 .. 65535)", n_kfs, max_kf_n);
    int rc = bowkf_check_record(ctx, kf1, "kf1");
    if (rc != ORBFE_OK) return rc;
    if (n_kfs == 0) return ORBFE_OK;
    hipStream_t s;
    rc = orbfe_enqueue_on(ctx, stream, false, &s);
    if (rc != ORBFE_OK) return rc;
    BowKfSearch a;
    rc = bowkf_fill(ctx, &a, kf1, n_kfs, max_kf_n, nnratio, check_ori, d_match12, d_pairs, d_nmatches, d_status);
    if (rc != ORBFE_OK) return rc;
    a.k2 = orbfe_bow_keyframe{}; // per record, on the device
    hipLaunchKernelGGL(bowkf_init_batch_kernel, dim3(a.k1.n > 0 ? (a.k1.n + 255) / 256 : 1, n_kfs), dim3(256), 0, s, a, d_kfs, max_kf_n);
    if (a.k1.nnodes > 0) hipLaunchKernelGGL(bowkf_node_match_batch_kernel, dim3((a.k1.nnodes + 3) / 4, n_kfs), dim3(256), 0, s, a, d_kfs, max_kf_n);
    hipLaunchKernelGGL(bowkf_tail_batch_kernel, dim3(n_kfs), dim3(1024), 0, s, a, d_kfs, max_kf_n);
    ORBFE_HIP_TRY(ctx, hipGetLastError());
    return ORBFE_OK;
} ORBFE_CATCH(ctx)
