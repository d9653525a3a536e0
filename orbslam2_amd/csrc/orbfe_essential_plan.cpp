// orbfe_essential_plan.cpp -- the host-only planner of orbfe_enqueue_optimize_essential_graph (orbfe_essential_graph.hip): from the edge
// list of Optimizer::OptimizeEssentialGraph to one relocatable blob of int32 words that the kernel follows without a host step.  No GPU
// call, no floating point: plain C++, testable on a CPU (tests/test_essential_graph_plan.py, tests/asan/essential_plan_harness.cpp).
//
// What the blob holds (every offset counts int32 words from the blob's start; orbfe_essential_plan_header in include/orbfe.h):
//   order[n_free]        elimination order: position -> keyframe.  Greedy minimum degree on the block graph of the free vertices (the
//                        degree is the number of not yet eliminated neighbours, fill included), ties to the lower keyframe index.
//   pos[n_kfs]           keyframe -> position, -1 for the fixed keyframe
//   colptr[n_free + 1], rowidx[n_lblocks]
//                        the block structure of L, fill included: column p holds the positions r > p, ascending.  Block k of rowidx
//                        is slot n_free + k; the diagonal block of position p is slot p.  A slot is 49 doubles, row major, and an
//                        off-diagonal slot (r, p) holds the block whose ROWS belong to position r.
//   edge_slots[n_edges][4]  per edge (i, j): slot of i's diagonal block, of j's, of the off-diagonal block, and the transposed flag
//                        (1 where order(i) > order(j): the stored block is Ji^T Jj, else Jj^T Ji).  -1 where there is none: an end
//                        that is the fixed keyframe, and all three for an edge left out (an end outside [0, n_kfs), or i == j).
//   slot_ptr[n_slots + 1], slot_edges[n_slot_edges]
//                        per slot the contributing edges in edge order as 2 * edge + side: on a diagonal slot side 0 = the edge's
//                        vertex 0 (Ji^T Ji), 1 = vertex 1; on an off-diagonal slot the transposed flag.  Duplicate pairs and both
//                        orientations of a pair share their slots.  Every H block is a sum in this order: no floating-point atomics.
//   upd_ptr[n_free + 1], upd[n_updates][3]
//                        per pivot p the updates of the right-looking factorisation: (slot of (r, p), slot of (c, p), target slot of
//                        (r, c)) for the rows r >= c of column p; the target of r == c is the diagonal slot r.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <set>
#include <vector>

#include "../../include/orbfe.h"

namespace {

int build_plan(int n_kfs, int fixed_kf, const int32_t *edge_i, const int32_t *edge_j, int n_edges, std::vector<int32_t> &out)
{
    if (n_kfs < 1 || n_edges < 0 || fixed_kf < 0 || fixed_kf >= n_kfs || (n_edges > 0 && (!edge_i || !edge_j))) return ORBFE_ERR_INVALID;
    const int n_free = n_kfs - 1;
    auto usable = [&](int e) { return edge_i[e] >= 0 && edge_i[e] < n_kfs && edge_j[e] >= 0 && edge_j[e] < n_kfs && edge_i[e] != edge_j[e]; };

    // the block graph of the free vertices
    std::vector<std::set<int32_t>> adj((size_t)n_kfs);
    for (int e = 0; e < n_edges; e++) {
        if (!usable(e) || edge_i[e] == fixed_kf || edge_j[e] == fixed_kf) continue;
        adj[edge_i[e]].insert(edge_j[e]);
        adj[edge_j[e]].insert(edge_i[e]);
    }
    // greedy minimum degree; the eliminated vertex's neighbours become a clique
    std::vector<int32_t> order((size_t)n_free), pos((size_t)n_kfs, -1);
    std::vector<std::vector<int32_t>> col((size_t)n_free);
    std::vector<uint8_t> gone((size_t)n_kfs, 0);
    gone[fixed_kf] = 1;
    for (int p = 0; p < n_free; p++) {
        int best = -1;
        for (int v = 0; v < n_kfs; v++)
            if (!gone[v] && (best < 0 || adj[v].size() < adj[best].size())) best = v;
        order[p] = best;
        pos[best] = p;
        gone[best] = 1;
        col[p].assign(adj[best].begin(), adj[best].end()); // keyframes for now
        for (int32_t u : col[p]) {
            adj[u].erase(best);
            for (int32_t w : col[p])
                if (w != u) adj[u].insert(w);
        }
        adj[best].clear();
    }
    std::vector<int32_t> colptr((size_t)n_free + 1, 0), rowidx;
    uint64_t n_updates64 = 0;
    for (int p = 0; p < n_free; p++) {
        for (int32_t &u : col[p]) u = pos[u];
        std::sort(col[p].begin(), col[p].end());
        rowidx.insert(rowidx.end(), col[p].begin(), col[p].end());
        colptr[p + 1] = (int32_t)rowidx.size();
        const uint64_t m = col[p].size();
        n_updates64 += m * (m + 1) / 2;
        if (rowidx.size() > (size_t)0x0fffffff || n_updates64 > (uint64_t)0x0fffffff) return ORBFE_ERR_UNSUPPORTED; // the blob would not fit int32
    }
    const int32_t n_lblocks = (int32_t)rowidx.size(), n_slots = n_free + n_lblocks, n_updates = (int32_t)n_updates64;
    auto lslot = [&](int32_t r, int32_t c) { // the slot of block (r, c), r > c: present by construction
        const int32_t *b = rowidx.data() + colptr[c], *e = rowidx.data() + colptr[c + 1];
        return n_free + (int32_t)(std::lower_bound(b, e, r) - rowidx.data());
    };

    std::vector<int32_t> edge_slots((size_t)n_edges * 4, -1), slot_cnt((size_t)n_slots + 1, 0);
    for (int e = 0; e < n_edges; e++) {
        if (!usable(e)) continue;
        int32_t *s = &edge_slots[(size_t)e * 4];
        const int32_t pi = pos[edge_i[e]], pj = pos[edge_j[e]];
        s[0] = pi; s[1] = pj;
        if (pi >= 0 && pj >= 0) { s[2] = pi > pj ? lslot(pi, pj) : lslot(pj, pi); s[3] = pi > pj ? 1 : 0; }
        for (int k = 0; k < 3; k++)
            if (s[k] >= 0) slot_cnt[s[k] + 1]++;
    }
    std::vector<int32_t> slot_ptr((size_t)n_slots + 1, 0);
    for (int s = 0; s < n_slots; s++) slot_ptr[s + 1] = slot_ptr[s] + slot_cnt[s + 1];
    const int32_t n_slot_edges = slot_ptr[n_slots];
    std::vector<int32_t> slot_edges((size_t)n_slot_edges), fill(slot_ptr.begin(), slot_ptr.end() - 1);
    for (int e = 0; e < n_edges; e++) {
        const int32_t *s = &edge_slots[(size_t)e * 4];
        if (s[0] >= 0) slot_edges[fill[s[0]]++] = 2 * e;
        if (s[1] >= 0) slot_edges[fill[s[1]]++] = 2 * e + 1;
        if (s[2] >= 0) slot_edges[fill[s[2]]++] = 2 * e + s[3];
    }
    std::vector<int32_t> upd_ptr((size_t)n_free + 1, 0), upd;
    upd.reserve((size_t)n_updates * 3);
    for (int p = 0; p < n_free; p++) {
        const int32_t b = colptr[p], m = colptr[p + 1] - b;
        for (int32_t x = 0; x < m; x++)
            for (int32_t y = 0; y <= x; y++) {
                const int32_t r = rowidx[b + x], c = rowidx[b + y];
                upd.push_back(n_free + b + x);
                upd.push_back(n_free + b + y);
                upd.push_back(r == c ? r : lslot(r, c));
            }
        upd_ptr[p + 1] = (int32_t)(upd.size() / 3);
    }

    orbfe_essential_plan_header h;
    memset(&h, 0, sizeof(h));
    h.magic = ORBFE_ESSENTIAL_PLAN_MAGIC;
    h.n_kfs = n_kfs; h.fixed_kf = fixed_kf; h.n_edges = n_edges; h.n_free = n_free; h.n_lblocks = n_lblocks;
    h.n_slot_edges = n_slot_edges; h.n_updates = n_updates;
    const std::vector<int32_t> *parts[9] = {&order, &pos, &colptr, &rowidx, &edge_slots, &slot_ptr, &slot_edges, &upd_ptr, &upd};
    int32_t *offs[9] = {&h.off_order, &h.off_pos, &h.off_colptr, &h.off_rowidx, &h.off_edge_slots, &h.off_slot_ptr, &h.off_slot_edges, &h.off_upd_ptr, &h.off_upd};
    uint64_t words = sizeof(h) / 4;
    for (int k = 0; k < 9; k++) { *offs[k] = (int32_t)words; words += parts[k]->size(); if (words > (uint64_t)0x1fffffff) return ORBFE_ERR_UNSUPPORTED; }
    h.blob_bytes = (int32_t)(words * 4);
    out.assign((size_t)words, 0);
    memcpy(out.data(), &h, sizeof(h));
    for (int k = 0; k < 9; k++)
        if (!parts[k]->empty()) memcpy(out.data() + *offs[k], parts[k]->data(), parts[k]->size() * 4);
    return ORBFE_OK;
}

} // namespace

extern "C" int orbfe_essential_graph_plan(int n_kfs, int fixed_kf, const int32_t *edge_i, const int32_t *edge_j, int n_edges, void *blob, size_t blob_capacity,
                                          size_t *blob_bytes)
{
    try {
        if (!blob_bytes) return ORBFE_ERR_INVALID;
        std::vector<int32_t> out;
        const int rc = build_plan(n_kfs, fixed_kf, edge_i, edge_j, n_edges, out);
        if (rc != ORBFE_OK) return rc;
        *blob_bytes = out.size() * 4;
        if (!blob || blob_capacity < *blob_bytes) return ORBFE_ERR_CAPACITY; // *blob_bytes says what is needed
        memcpy(blob, out.data(), *blob_bytes);
        return ORBFE_OK;
    } catch (...) {
        return ORBFE_ERR_HIP; // out of host memory
    }
}

extern "C" int orbfe_essential_graph_plan_size(int n_kfs, int fixed_kf, const int32_t *edge_i, const int32_t *edge_j, int n_edges, size_t *blob_bytes)
{
    const int rc = orbfe_essential_graph_plan(n_kfs, fixed_kf, edge_i, edge_j, n_edges, nullptr, 0, blob_bytes);
    return rc == ORBFE_ERR_CAPACITY ? ORBFE_OK : rc;
}
