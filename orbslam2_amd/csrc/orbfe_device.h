// orbfe_device.h -- device-side configuration shared by the kernels and the host API.
// gfx950 only (wave64).  See DESIGN.md for the HBM layout.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "orbfe_config.h"

typedef unsigned long long u64; // a wave's ballot, a lane's 64 flags

// Profiling cut points (tools/*_phases.sh, tools/*_insts.sh): an extra kernel argument that makes a kernel return after a
// given phase so that phases can be timed / counted.  They exist ONLY in the -DORBFE_PROFILE_CUTS build (make cuts ->
// tools/ab/cuts.so); the shipped liborbfe.so has neither the argument nor the branches nor the getenv.
#ifdef ORBFE_PROFILE_CUTS
#define ORBFE_CUT_PARAM , int dbg
// the marker leaves "; ORBFE_PHASE_END n" in the kernel's assembly at the cut: tools/isa_mix.py splits the disassembly into phases there
template <int N> __device__ __forceinline__ bool orbfe_phase_end() { asm volatile("; ORBFE_PHASE_END %0" ::"n"(N)); return true; }
#define ORBFE_CUT(n) (orbfe_phase_end<n>() && dbg == (n))
#define ORBFE_CUT_ARG(env) , orbfe_cut_value(env)
static inline int orbfe_cut_value(const char *env) { const char *v = getenv(env); return v ? atoi(v) : 0; }
#else
#define ORBFE_CUT_PARAM
#define ORBFE_CUT(n) false
#define ORBFE_CUT_ARG(env)
#endif

// Per-batch device buffers (all [image][...] with the per-image strides of DeviceConfig).
struct DeviceBuffers {
    uint8_t *pyr;        // raw pyramid
    // Level 0 as the kernels read it (level_image(), orbfe_common.hpp).  Copy mode: pyr + lv[0].pyr_off, per-image stride pyr_bytes,
    // pitch lv[0].pitch, reflect-101 margin materialised by ingest.  In-place mode (lv0_packed = 1, round 4): the caller's packed
    // CV_8UC1 images themselves -- no ingest launch, no copy; rows at any alignment, no margin (the blur of level 0 reflects by
    // itself, every other reader stays inside the image)
    const uint8_t *lv0;
    size_t lv0_stride;
    int lv0_pitch, lv0_packed;
    uint8_t *blur;       // blurred pyramid
    int *cell_cnt;       // [img][cells_total]
    uint32_t *cell_xy;   // [img][cells_total*cell_cap]  x | y<<16 (region relative)
    uint8_t *cell_sc;    // [img][cells_total*cell_cap]
    int *cell_base;      // [img][cells_total] scratch (exclusive scan)
    uint32_t *cand_xy;   // [img][cand_total]
    uint8_t *cand_sc;    // [img][cand_total]
    uint32_t *ot_xy2;    // [img][cand_total] quadtree ping-pong partner
    uint32_t *idx0, *idx1; // [img][cand_total] ping-pong permutation
    uint32_t *bk_part;   // [img][bk_part_total] count | best slot << 12 | best score << 24 (ORBFE_BK_PART) of every bucket a FAST cell's
                         // survivors can fall into, cell after cell; rewritten by fast_cell_kernel every frame, summed into the
                         // bucket arrays (LDS) by octree3_kernel
    int *bk_end;         // [img][nlevels][4097] quadtree deep path: bucket ends of the counting sort
    uint8_t *ot3_scratch; // [img][nlevels][node_bytes] quadtree node tables when they do not fit LDS (else null)
    uint32_t *bk_best;   // [img][nlevels][ORBFE_BK_PYR] best-key pyramid of every (image, level): written after the pyramid step, read by the final selection
    int *lvl_ncand;      // [img][nlevels]
    int *sel_cnt;        // [img][nlevels]
    uint32_t *sel_xy;    // [img][sel_total]
    uint8_t *sel_sc;     // [img][sel_total]
    uint32_t *proc_xy;   // [img][sel_total] describe_kernel's processing order (DeviceConfig::proc_order): the keypoints of a level in a spatial order, ...
    uint32_t *proc_meta; // ... and their slot | score << 24 (octree3_kernel writes both beside sel_xy / sel_sc, which stay in the reference's order)
    void *kps;           // [img][sel_total] orbfe_keypoint
    uint8_t *desc;       // [img][sel_total][32]
    int *kp_cnt;         // [img]
    float *u_right;      // [img][sel_total]
    float *depth;        // [img][sel_total]
    int *sad;            // [img][sel_total] best SAD (or -1)
    int *status;         // [img] non-zero = device-side capacity problem
    int *row_cnt;        // [pair][height] stereo row lists: right keypoints whose band covers the row (every row written by the row-list waves, orbfe_rowlist.hpp)
    uint2 *row_ent;      // [pair][height][row_cap] entries: (iR | octave << 16, x bits), written by stereo_rowlist_kernel
    const uint32_t *bk_tab; // quadtree bucket tables: per level X[region_w] then Y[region_h] (see ORBFE_BK_*)
    const uint32_t *bk_emap; // [bk_part_total] bucket index | level-local cell << 16 of every bk_part entry
    const uint32_t *bk_off;  // [cells_total] first bk_part entry of the cell; ~0u: the cell spans > 64 buckets (no partials)
    const uint32_t *rs_tab; // cv::resize offset/weight tables of every level (see pyr_resize_kernel)
    const uint4 *cell_info; // [cells_total] FAST cells: level | valid << 8, ini_x | ini_y << 16, tile w | h << 8, index inside the level (fast_cell_kernel)
    const uint2 *cell_aux;  // [cells_total] the lane maps of the cell's shape, divided on the host: x = shape index (fast_lane_tab) | (64 / ng) << 17 | last band's first row << 24
                            // (ng = 4-pixel groups per interior row), y = ceil(2^16 / cpr) | (64 / cpr) << 17 (cpr = 16-byte chunks per tile row)
    const uint32_t *fast_lane_tab; // [shapes][64 lanes][8]: phase A's per-lane constants of a cell shape (tile w x h): pixel masks of the pairs 0 1 / 2 3, the same in
                                   // the cell's last band, entry word of pixels 0 1, word offset of the lane's window in the LDS tile, 2 spare
    const uint32_t *blur_tile_info; // [blur_tiles_total] level | column strip << 8 | first row << 16 (blur_kernel)
    const uint32_t *rs_blk; // per (level, block of 4 * rs_rw output rows): first source row | source rows << 16 (pyr_resize_kernel)
    const int *pair_plan;   // pyr_pair_kernel: per tile column / row of a level pair {first word (row) of the LDS tile, words (rows), first, end word (row) this workgroup stores}
    const int *tail_plan;   // [tail_strips][ORBFE_TAIL_MAX][4]: first extended column, words, first staged source column, staged words (pyr_tail_kernel)
    long long *dbg_ts;   // 4096 timestamps for kernel bring-up (ORBFE_OT2_STOP=99); never read by product code
    const uint8_t *slot_level; // [sel_total] level of every keypoint slot
    const int16_t *patch_uv; // IC_Angle patch offsets: (u & 0xff) | (v << 8), padded with (0,0)
    const uint32_t *mom_tab; // [64 lanes][12] byte-dot-product weights of the same patch (hp == 15), see orbfe_plan.cpp
    const uint32_t *pattern; // [256] the extractor's copy of the rBRIEF tests (src/ORBextractor.cc:442-444): x0 | y0 << 8 | x1 << 16 | y1 << 24 as int8;
                             // the compiled bit_pattern_31_ unless orbfe_set_pattern replaced it
    uint8_t *otg_scratch;    // [img][orbfe_otg_level_off(cfg, nlevels)] node tables of octree_generic_kernel<true>, level after level (else null)
};

struct KeyPointPOD {
    float x, y, size, angle, response;
    int32_t octave, class_id;
};
static_assert(sizeof(KeyPointPOD) == 28, "keypoint must match cv::KeyPoint");

// launchers (orbfe_pyramid.hip, orbfe_fast.hip, orbfe_octree*.hip, orbfe_describe.hip, orbfe_stereo.hip)
void orbfe_launch_ingest(const DeviceConfig &cfg, const DeviceBuffers &buf, const uint8_t *d_images,
                         int n_images, hipStream_t s);
int orbfe_launch_pyramid(const DeviceConfig &cfg, const DeviceBuffers &buf, int n_images, bool fuse_blur, hipStream_t s, int ride_from = ORBFE_MAX_LEVELS); // returns the number of levels (from 0) whose blur it launched too
void orbfe_launch_blur(const DeviceConfig &cfg, const DeviceBuffers &buf, int n_images, int first_level, hipStream_t s);
hipError_t orbfe_launch_fast(const DeviceConfig &cfg, const DeviceBuffers &buf, int n_images, bool buckets, hipStream_t s, const FastRange &r); // an empty range launches nothing; hipErrorInvalidValue: a range the launch cannot state
// orbfe_octree_generic.hip: nodes_in_hbm selects octree_generic_kernel<true> (node tables in DeviceBuffers::otg_scratch); the error of a
// refused LDS attribute is returned and nothing is launched
hipError_t orbfe_launch_octree_generic(const DeviceConfig &cfg, const DeviceBuffers &buf, int n_images, bool nodes_in_hbm, hipStream_t s);
int orbfe_octree_generic_prepare(const DeviceConfig &cfg, bool nodes_in_hbm);
// orbfe_octree3.hip
void orbfe_launch_octree3(const DeviceConfig &cfg, const DeviceBuffers &buf, int n_images, int sort_cap, size_t lds, bool nodes_in_hbm, hipStream_t s);
void orbfe_launch_candidates_gather(const DeviceConfig &cfg, const DeviceBuffers &buf, int n_images, hipStream_t s);
int orbfe_octree3_prepare(size_t lds, bool nodes_in_hbm);
void orbfe_launch_describe(const DeviceConfig &cfg, const DeviceBuffers &buf, int n_images, bool stereo, hipStream_t s);
void orbfe_launch_stereo_rowlists(const DeviceConfig &cfg, const DeviceBuffers &buf, int n_pairs, hipStream_t s);
void orbfe_launch_stereo_match(const DeviceConfig &cfg, const DeviceBuffers &buf, int n_pairs, hipStream_t s);
void orbfe_launch_stereo_median(const DeviceConfig &cfg, const DeviceBuffers &buf, int n_pairs, hipStream_t s);
void orbfe_launch_rgbd(const DeviceConfig &cfg, const DeviceBuffers &buf, const float *d_depth,
                       size_t depth_pitch_floats, int image, hipStream_t s);
void orbfe_launch_undistort(const DeviceConfig &cfg, const void *d_keys_in, void *d_keys_out, int n, hipStream_t s);
struct GridFrame; // orbfe_match_window.hpp
void orbfe_launch_grid_build(const GridFrame &f, hipStream_t s); // Frame::AssignFeaturesToGrid into f.cell_off / f.cell_idx (orbfe_match_device.hip)
struct orbfe_context;
struct orbfe_grid_keyframe;
// the GridFrame of a keyframe record, its count and bounds checked (orbfe_fuse_device.hip); ORBFE_ERR_INVALID through orbfe_fail
int orbfe_grid_frame_of_record(orbfe_context *ctx, const orbfe_grid_keyframe *kf, GridFrame &f);
void orbfe_launch_rgbd_u16(const DeviceConfig &cfg, const DeviceBuffers &buf, const uint16_t *d_depth, size_t depth_pitch_px,
                           float factor, int image, hipStream_t s);
void orbfe_launch_rgbd_batch(const DeviceConfig &cfg, const DeviceBuffers &buf, const void *d_depth, bool is_u16, float factor, int n_images, hipStream_t s);
// byte offsets of the arrays inside a packed result block (orbfe_packed_layout of include/orbfe.h mirrors it)
struct PackedOffsets { size_t counts, level_counts, xy, angle, response, desc, u_right, depth; };
void orbfe_launch_pack_results(const DeviceConfig &cfg, const DeviceBuffers &buf, uint8_t *d_out, const PackedOffsets &lay, int n_out, int img_step, bool stereo, hipStream_t s);
