// orbfe_bow_vocab.h -- what the two bag-of-words translation units share: the resident fbow vocabulary (orbfe_bow.hip loads
// it, orbfe_bow_device.hip reads it) and the descent of one descriptor through it.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>

#include "orbfe_host.h"

#define BOW_MAX_DEPTH 32 // node ids are 32-bit paths of ceil(log2 k) bits per level: deeper trees cannot be addressed anyway

struct FbowParams { // fbow::Vocabulary::params, Thirdparty/fbow/src/fbow.h:118-129
    char desc_name[50];
    uint32_t aligment, nblocks;
    uint64_t desc_size_bytes_wp, block_size_bytes_wp, feature_off_start, child_off_start, total_size;
    int32_t desc_type, desc_size;
    uint32_t m_k;
};
static_assert(sizeof(FbowParams) == 120, "fbow params layout");

struct orbfe_bow_state {
    FbowParams p;
    uint8_t *d_data = nullptr;
    bool loaded = false;
    void *d_scratch = nullptr;
    size_t scratch_bytes = 0;
    DevBuf resident; // scratch of the asynchronous calls on a resident frame (orbfe_bow_device.hip): grow-only, never shared with d_scratch
    // keyframe database (KeyFrameDatabase): BoW vectors of the keyframes, resident in HBM, CSR by keyframe
    uint32_t *d_db_words = nullptr;
    float *d_db_w = nullptr;
    size_t db_cap = 0;                 // entries allocated
    std::vector<int> db_off, db_len;   // per keyframe: first entry, number of words (0 after erase)
    std::vector<uint8_t> db_dead;      // erased keyframes: never scored again, their words are reclaimed by kfdb_compact
    size_t db_used = 0;
    size_t db_dead_words = 0;          // words of erased keyframes still occupying the CSR
    ~orbfe_bow_state()
    {
        if (d_data) hipFree(d_data);
        if (d_scratch) hipFree(d_scratch);
        if (d_db_words) hipFree(d_db_words);
        if (d_db_w) hipFree(d_db_w);
    }
};

// the tree as a kernel argument
struct BowTree {
    const uint8_t *data;
    unsigned block_size, feat_off, child_off, desc_wp;
    int nbits; // ceil(log2 k): bits of a node id per level
};

// fbow::Vocabulary::_transform2 for one descriptor: descend by minimum Hamming distance (first minimum wins) to a leaf;
// word id, weight and the id of the node passed at `store_level` (the leaf's parent path when the tree is shallower).
__device__ __forceinline__ void bow_walk(const BowTree &t, int store_level, const uint8_t *__restrict__ desc32, uint32_t &wid, float &w, uint32_t &nid)
{
    unsigned long long feat[4];
    {
        const unsigned long long *p = (const unsigned long long *)desc32;
#pragma unroll
        for (int i = 0; i < 4; i++) feat[i] = p[i];
    }
    const uint8_t *blk = t.data;
    uint32_t level = 0, cur_node = 0;
    nid = 0; wid = 0; w = 0.f;
    for (;;) {
        const int N = *(const uint16_t *)blk;
        unsigned best_d = 0xffffffffu, best_i = 0;
        for (int c = 0; c < N; c++) {
            const unsigned long long *nf = (const unsigned long long *)(blk + t.feat_off + (size_t)c * t.desc_wp);
            const unsigned d = __popcll(nf[0] ^ feat[0]) + __popcll(nf[1] ^ feat[1]) + __popcll(nf[2] ^ feat[2]) + __popcll(nf[3] ^ feat[3]);
            if (d < best_d) { best_d = d; best_i = (unsigned)c; }
        }
        if (level == (uint32_t)store_level) nid = cur_node;
        const uint32_t id_or_child = *(const uint32_t *)(blk + t.child_off + (size_t)best_i * 8);
        if (id_or_child & 0x80000000u) {
            wid = id_or_child & 0x7fffffffu;
            w = *(const float *)(blk + t.child_off + (size_t)best_i * 8 + 4);
            if (level < (uint32_t)store_level) nid = cur_node;
            break;
        }
        const uint32_t child = id_or_child & 0x7fffffffu;
        blk = t.data + (size_t)child * t.block_size;
        cur_node = (cur_node << t.nbits) | best_i;
        level++;
        if (child == 0 || level > BOW_MAX_DEPTH) break; // orbfe_vocab_load rejects deeper / cyclic trees; never spin on a bad blob
    }
}
