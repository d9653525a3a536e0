// orbfe_config.h -- what the kernels and the host planner (orbfe_plan.cpp) share: per-level geometry, DeviceConfig (passed to every
// kernel by value), the pure size / index helpers.  No HIP header (the planner is plain C++); __host__ __device__ where a kernel calls.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define ORBFE_HD __attribute__((host, device)) inline __attribute__((always_inline)) // __host__ __device__ __forceinline__, spelt without the HIP headers
#else
#define ORBFE_HD inline
#endif

#define ORBFE_MAX_LEVELS 16
#define ORBFE_TAIL_MAX 3   // levels fused by pyr_tail_kernel
#define ORBFE_TAIL_COLS 64 // extended columns of the last level per workgroup
#ifndef ORBFE_BLUR_ROWS
#define ORBFE_BLUR_ROWS 32
#endif
#define ORBFE_WAVE 64
#define PYR_MX 4 // reflect-101 margin of every pyramid level: pixels left of column 0 ...
#define PYR_MY 3 // ... and rows above row 0 / below the last row
#ifndef ORBFE_PYR_RB
#define ORBFE_PYR_RB 4 // extended rows per wave of pyr_resize_direct_kernel (0: never use it; A/B builds only)
#endif
// Per-level geometry (reference: src/ORBextractor.cc:759-781,925-926,533-557).
struct LevelInfo {
    int w, h, pitch;       // level image size and row pitch (bytes)
    int pyr_off;           // byte offset of the level inside one image's pyramid buffer
    int n_cols, n_rows;    // FAST cell grid
    int w_cell, h_cell;
    int cell_off, n_cells; // cell index range inside one image's cell arrays
    int quota;             // mnFeaturesPerLevel[level]
    int n_ini;             // quadtree roots
    float hx;              // root width (float, as the reference)
    int cand_off, cand_cap;// candidate array range inside one image's candidate arrays
    int sel_off, sel_cap;  // selected-keypoint slot range inside one image's slot arrays
    int blur_off, blur_tx; // blurred level: byte offset inside one image's blurred pyramid and 32-px tiles per tile row (tiled layout)
    int blur_tile_off;     // first blur tile of this level in the fused all-level grid
    int blur_tiles_x, blur_tiles_y;
    int scaled_patch;      // int(patchSize * scale)
    float scale, inv_scale;
    double rs_scale_x, rs_scale_y; // cv::resize scale from level-1 (1/(dw/sw))
    int rs_xtab_off, rs_xtab_n;    // resize column table (two planes of rs_xtab_n words) in DeviceBuffers::rs_tab
    int rs_ytab_off, rs_ytab_n;    // resize row table
    int rs_src_rows[3];            // source rows spanned by the worst block of 16 / 8 / 4 output rows (pyr_resize_kernel)
    int rs_rw, rs_blk_off;         // rows per wave the launch uses (4 / 2 / 1) and this level's entries in DeviceBuffers::rs_blk
    int rs_direct, rs_dtab_off;    // pyr_resize_direct_kernel usable (every 4-column word's sources lie within 8 bytes) and its table: rs_xtab_n byte selectors, then rs_xtab_n / 4 first-source-byte offsets
    // pyr_pair_kernel (this level and the next in one launch): usable, tile grid over the NEXT level's extended domain (tiles of
    // pp_tw words x pp_tr rows), and this level's entries in DeviceBuffers::pair_plan (int4 units)
    int pp_ok, pp_ntx, pp_nty, pp_tw, pp_tr, pp_xoff, pp_yoff;
    int bk_xoff, bk_yoff;          // quadtree bucket tables of this level in DeviceBuffers::bk_tab (orbfe_octree3.hip)
    int bk_part_off, bk_part_n;    // this level's per-cell bucket partials in DeviceBuffers::bk_part / bk_emap
    int bk_depth;                  // quadtree bucket depth of this level: 5, or 4 where a FAST cell would span more than 64 depth-5 buckets
    int po_rb, po_cb;              // processing order: row / column bits of a node's bin (orbfe_octree3.hip step 4a)
    int bk_points;                 // some cell of the level spans > 64 buckets: the quadtree kernel buckets its candidates itself
};

struct DeviceConfig {
    int nlevels;
    int width, height;
    int edge_threshold, min_border; // min_border = edge_threshold - 3
    int ini_th, min_th;
    uint32_t ini_th_h2, min_th_h2; // the thresholds as half-precision numbers in both halves of a word (fast_cell_kernel's score clamp)
    int half_patch;
    int cell_cap;          // slots per FAST cell
    int cells_total;       // per image
    int cand_total;        // per image
    int sel_total;         // per image == keypoint capacity
    int blur_tiles_total;
    int proc_order;        // octree3_kernel also writes proc_xy / proc_meta and describe_kernel walks those (0: describe_kernel walks sel_xy; ORBFE_NO_PROC_ORDER=1, other quadtree kernels)
    int fast_blur_t0;      // blur tiles [fast_blur_t0, blur_tiles_total) ride in the FAST launch (set per launch; blur_tiles_total: none);
                           // negative: the prefix [0, -fast_blur_t0) rides (fast_range_decode)
    uint32_t xcd_magic;    // ceil(2^32 / workgroups per XCD and round of units) of the block map of the launch this copy is passed to (FAST, describe,
                           // stereo match: set by the launcher, xcd_map_magic_host; 0: divide in the kernel)
    int max_nodes;         // quadtree node capacity (LDS)
    int bk_part_total;     // per image: entries of DeviceBuffers::bk_part
    int row_cap;           // entries per image row in DeviceBuffers::row_ent
    int patch_n;           // entries in DeviceBuffers::patch_uv (multiple of 64)
    // fused pyramid tail (pyr_tail_kernel): the last tail_n levels (2 or 3) in one launch, 0 = not used
    int tail_first, tail_n, tail_strips;
    int pp_max_images;                 // pyr_pair_kernel (two levels per launch) serves batches of up to this many images
    int tail_max_images;               // the fused tail serves batches of up to this many images; larger ones run levels tail_first.. as single launches
    int tail_src_words;                // staged words per row of level tail_first - 1 (widest strip)
    int tail_words[ORBFE_TAIL_MAX];    // words per row of stage s computed by the widest strip
    int tail_lds_y[ORBFE_TAIL_MAX];    // LDS byte offsets: row tables of stage s, ...
    int tail_lds_buf[ORBFE_TAIL_MAX];  // ... and the columns of stage s kept for stage s + 1
    int tail_lds_src, tail_lds_bytes;
    int umax[64];
    int taps[7];           // Gaussian 8.8 fixed-point taps
    size_t pyr_bytes;      // per image
    size_t blur_bytes;     // per image: blurred pyramid, 32 x 4 px tiles of 128 B, each eight 4 x 4 px blocks (see orbfe_pyramid.hip)
    float bf, fx, mb;
    // input pixel format (orbfe_set_input_format): 1 = CV_8UC1; 3 / 4 = interleaved colour converted by ingest with
    // cv::cvtColor's fixed-point weights for channels 0, 1, 2 (in_coef) and in_shift fraction bits
    int in_cn, in_coef[3], in_shift;
    size_t in_image_bytes; // bytes of one packed input image (w * h * in_cn, or rm_sw * rm_sh with rectification)
    // rectification (orbfe_set_rectification): cv::remap's fixed-point form of the float maps, one pair per side
    // (index = image slot & 1 when the right map is set, else 0): rm_xy = sx | sy << 16 (int16 each), rm_a = fy * 32 + fx
    int rm_on, rm_sw, rm_sh;
    // cells [fast_cell_c0, cells_total) run in the FAST launch this copy is passed to; negative: the prefix [0, -fast_cell_c0)
    // (set per launch like fast_blur_t0; 0 = every cell, which is what the planner leaves here).  It fills the four bytes that
    // aligned rm_xy, so the layout every kernel reads is unchanged.
    int fast_cell_c0;
    const uint32_t *rm_xy[2];
    const uint16_t *rm_a[2];
    // lens distortion of Frame::UndistortKeyPoints (orbfe_set_distortion): k1 k2 p1 p2 k3; n_dist == 0 or dist[0] == 0: none
    int n_dist;
    float dist[5];
    float cam[4];          // fx fy cx cy
    LevelInfo lv[ORBFE_MAX_LEVELS];
};
// DeviceConfig is a kernel argument: the host planner and every kernel must agree on it byte for byte
static_assert(sizeof(LevelInfo) == 224 && sizeof(DeviceConfig) == 4168, "LevelInfo / DeviceConfig layout changed");
static_assert(offsetof(DeviceConfig, pyr_bytes) == 440 && offsetof(DeviceConfig, rm_xy) == 512 && offsetof(DeviceConfig, lv) == 584,
              "DeviceConfig layout changed");
static_assert(offsetof(DeviceConfig, fast_cell_c0) == 508, "DeviceConfig layout changed");

// The range words of a FAST launch (DeviceConfig::fast_cell_c0 / fast_blur_t0): one word states a suffix [v, total) (v >= 0) or a
// prefix [0, -v) (v < 0) of the cell table / the blur tile table, which is what a launch plan cut at a level boundary needs.
struct FastRange { int c0, c1, t0, t1; }; // cells [c0, c1) and riding blur tiles [t0, t1) of one FAST launch
ORBFE_HD void fast_range_decode(int v, int total, int &lo, int &hi) { lo = v < 0 ? 0 : v; hi = v < 0 ? -v : total; }
// the word for [lo, hi) of [0, total); false when the range is neither a prefix, a suffix nor empty
static inline bool fast_range_encode(int lo, int hi, int total, int *v)
{
    if (lo >= hi) { *v = total; return true; } // empty: the suffix that starts at the end
    if (hi == total) { *v = lo; return true; }
    if (lo == 0) { *v = -hi; return true; }
    return false;
}

// Quadtree buckets (orbfe_octree3.hip).  A candidate's bucket = its root and quadrant path down to depth 5; the
// path is separable (x decides the x bits, y the y bits), so it is X[x] | Y[y] from two host-built tables:
//   X[x] = root << 10 | x bits spread to the even positions | (root * 32 + column) << 16
//   Y[y] = y bits spread to the odd positions | row << 16
// Best key of a bucket: score (8 bits) << 24 | ~(level-local cell (12 bits) << 12 | slot (12 bits)) -- maximum
// = best score, first in cv::FAST emission order.
#define ORBFE_BK_DEPTH 5
#define ORBFE_BK_BUCKETS 4096
#define ORBFE_BK_PYR 5460 // entries of one bucket pyramid: 4 roots x (1 + 4 + ... + 4^5)
#define ORBFE_BK_REF_MASK 0xffffffu
#define ORBFE_BK_KEY(sc, cell, slot) (((sc) << 24) | (ORBFE_BK_REF_MASK - (unsigned)(((cell) << 12) | (slot))))
// A cell's partial entry: the cell is implied by the entry's position, so count (<= cell_cap <= 1024) and the key's score and
// (inverted) slot fields fit one word; ORBFE_BK_PART_KEY rebuilds the key for level-local cell `cell`.
#define ORBFE_BK_PART(cnt, key) ((cnt) | (((key) & 0xfffu) << 12) | ((key) & 0xff000000u))
#define ORBFE_BK_PART_KEY(e, cell) (((e) & 0xff000000u) | ((4095u - (unsigned)(cell)) << 12) | (((e) >> 12) & 0xfffu))

// bucket-pyramid quadtree (orbfe_octree3.hip): its count / best-key pyramids size the LDS the planner budgets
#define OT3_ROOTS 4                    // root slots per level (n_ini <= 4)
#define OT3_PYR (OT3_ROOTS * 1365)     // sum_{d=0..5} 4^d = 1365 entries per root
#define OT3_HI (OT3_ROOTS * 85)        // entries of depths 0..3 (32-bit counts); depths 4 and 5 follow as 16-bit counts

// first source column of extended column i (cv::resize's xofs, as the planner builds the table; it checks this formula against it)
ORBFE_HD int resize_first_source(int dx, double scale, int src_w)
{
    const float fx = (float)(((double)dx + 0.5) * scale - 0.5);
    int sx = (int)floorf(fx);
    sx = sx < 0 ? 0 : sx;
    return sx >= src_w - 1 ? src_w - 1 : sx;
}
ORBFE_HD int resize_word_base(int xw, int dst_w, double scale, int src_w)
{
    int lo = 0x7fffffff;
    for (int j = 0; j < 4; j++) {
        int q = 4 * xw + j - PYR_MX;
        if (dst_w == 1) q = 0;
        else while (q < 0 || q >= dst_w) q = q < 0 ? -q : 2 * dst_w - 2 - q;
        lo = q < lo ? q : lo;
    }
    return resize_first_source(lo, scale, src_w);
}

static inline int max_cell_w(const DeviceConfig &cfg) { int m = 0; for (int l = 0; l < cfg.nlevels; l++) m = cfg.lv[l].w_cell > m ? cfg.lv[l].w_cell : m; return m; }
// bytes per row of fast_cell_kernel's LDS tile (the planner builds fast_lane_tab with it)
static inline int orbfe_fast_tile_pitch(const DeviceConfig &cfg) { return (max_cell_w(cfg) + 6 + 15) & ~15; } // whole 16-byte chunks (the staging stores 128 bits at a time)

// the quadtree kernels' sort buffer: a power of two >= max_nodes
static inline int orbfe_sort_cap(int max_nodes) { int p = 1; while (p < max_nodes) p <<= 1; return p; }

// bytes of one node array: three words per node, and room for the sort keys of the "largest node first" phase, which are built
// in the array that is not in use (the next pass's nodes are written after the ranking)
ORBFE_HD size_t ot3_slot_bytes(int cap, int sort_cap)
{
    const size_t a = 3 * sizeof(int) * (size_t)cap, k = sizeof(unsigned long long) * (size_t)sort_cap;
    return ((a > k ? a : k) + 15) & ~(size_t)15;
}
// bytes of the node tables (two node arrays, per-node bookkeeping) of one workgroup
static inline size_t orbfe_octree3_node_bytes(int max_nodes, int sort_cap)
{
    const size_t cap = (size_t)max_nodes;
    return ((2 * ot3_slot_bytes(max_nodes, sort_cap) + sizeof(int) * cap * (4 + 1 + 1 + 1 + 1) + 64) + 255) & ~(size_t)255;
}
// dynamic LDS of octree3_kernel: the count pyramid (32-bit entries for depths 0..3, 16-bit for depths 4 and 5), then one region
// that holds the best-key pyramid while the buckets are summed up and the node tables afterwards (unless those live in HBM)
static inline size_t orbfe_octree3_lds_bytes(int max_nodes, int sort_cap, bool nodes_in_hbm)
{
    const size_t cnt = sizeof(int) * OT3_HI + sizeof(uint16_t) * (OT3_PYR - OT3_HI), best = sizeof(int) * OT3_PYR;
    const size_t nodes = nodes_in_hbm ? 0 : orbfe_octree3_node_bytes(max_nodes, sort_cap);
    return ((cnt + 15) & ~(size_t)15) + (best > nodes ? best : nodes) + 64;
}
// dynamic LDS of octree_generic_kernel (orbfe_octree_generic.hip)
static inline size_t orbfe_octree_lds_bytes(const DeviceConfig &cfg)
{
    const int cap = cfg.max_nodes;
    const size_t node = 2 * sizeof(int) * cap + 4 * sizeof(short) * cap + ((cap + 7) / 8) * 8;
    return sizeof(unsigned long long) * orbfe_sort_cap(cfg.max_nodes) + 2 * node + sizeof(int) * 4 * cap + 4 * sizeof(int) * cap;
}
// octree_generic_kernel<true>: the same tables in HBM scratch, one region per (image, level) sized by the level's own node capacity
// (sel_cap + 1 >= max(quota + 3, 4 * n_ini) + 2 nodes, the bound max_nodes states for the largest level) and the power of two above it
ORBFE_HD int orbfe_otg_level_cap(const DeviceConfig &cfg, int level) { return cfg.lv[level].sel_cap + 1; }
ORBFE_HD int orbfe_otg_sort_cap(int cap) { int p = 1; while (p < cap) p <<= 1; return p; }
ORBFE_HD size_t orbfe_otg_level_bytes(const DeviceConfig &cfg, int level)
{
    const size_t cap = (size_t)orbfe_otg_level_cap(cfg, level);
    const size_t node = 2 * sizeof(int) * cap + 4 * sizeof(short) * cap + ((cap + 7) / 8) * 8;
    const size_t b = sizeof(unsigned long long) * (size_t)orbfe_otg_sort_cap((int)cap) + 2 * node + sizeof(int) * 4 * cap + 4 * sizeof(int) * cap;
    return (b + 255) & ~(size_t)255;
}
// byte offset of level `level`'s region inside one image's scratch; level == nlevels: the bytes of one image
ORBFE_HD size_t orbfe_otg_level_off(const DeviceConfig &cfg, int level)
{
    size_t off = 0;
    for (int l = 0; l < level; l++) off += orbfe_otg_level_bytes(cfg, l);
    return off;
}
