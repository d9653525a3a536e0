// orbfe_plan.h -- the host half of orbfe_create: every table and launch plan of a context, computed from its parameters
// alone.  Plain C++ (no HIP call, no environment read), so tests/asan/plan_harness.cpp runs the very code the library does.
#pragma once

#include "../../include/orbfe.h"
#include "orbfe_config.h"

#include <vector>

// The environment knobs of the launch plan, read once per context by from_env().  Each selects an
// alternative plan with identical results.
struct PlanKnobs {
    bool no_inplace = false;    // ORBFE_NO_INPLACE=1: level 0 copied by ingest
    int no_pair = -1;           // ORBFE_NO_PAIR: 1 = no pyr_pair_kernel, 0 = pairs at every batch size, -1 = unset
    int no_tail = -1;           // ORBFE_NO_TAIL: 1 = no pyr_tail_kernel, 0 = the tail at every batch size, -1 = unset
    bool pyr_lds = false;       // ORBFE_PYR_LDS=1: LDS-staged resize on every level
    bool no_fuse = false;       // ORBFE_NO_FUSE=1: blur in launches of its own
    bool no_proc_order = false; // ORBFE_NO_PROC_ORDER=1: describe_kernel walks the slots
    bool octree_generic = false;// ORBFE_OCTREE=1: the generic node-parallel quadtree kernel, node tables in LDS
    bool octree_generic_hbm = false; // ORBFE_OCTREE=2: the generic quadtree kernel, node tables in HBM scratch
    int blur_ride_from = -1;    // ORBFE_BLUR_RIDE_FROM=<n>: first level whose blur rides in FAST's launch, for every batch size
    int fast_split = -1;        // ORBFE_FAST_SPLIT: 1 = FAST's level 0 on the side stream at every batch size, 0 = never, -1 = unset
    bool host_trace = false;    // ORBFE_HOST_TRACE set: print the plan's choices to stderr
    static PlanKnobs from_env();
};

// What the launchers read besides DeviceConfig (orbfe_context keeps a copy).
struct LaunchPlan {
    float scale[ORBFE_MAX_LEVELS], inv_scale[ORBFE_MAX_LEVELS], sigma2[ORBFE_MAX_LEVELS], inv_sigma2[ORBFE_MAX_LEVELS];
    int32_t feats[ORBFE_MAX_LEVELS];
    bool use_octree3 = false;      // bucket-pyramid quadtree (orbfe_octree3.hip); preferred when its limits hold
    size_t ot3_lds = 0;
    bool ot3_nodes_in_hbm = false; // node tables of the bucket-pyramid quadtree in HBM scratch (large per-level quotas)
    int ot_sort_cap = 0;           // power of two >= max_nodes: the quadtree kernels' sort buffer
    bool otg_nodes_in_hbm = false; // generic quadtree kernel (use_octree3 false): node tables in HBM scratch (they exceed 150 KB of LDS, or ORBFE_OCTREE=2)
    size_t otg_scratch_bytes = 0;  // ... and that scratch's bytes per image (orbfe_otg_level_off(cfg, nlevels)), 0 when not used
    bool fuse_blur = true;         // blur level l - 1 in the launch that resizes it into level l (ORBFE_NO_FUSE=1: separate launches)
    // The blur of level l only needs level l, is memory-bound and is first read by describe_kernel: levels >= blur_ride_from are
    // blurred by workgroups that ride in FAST's launch (issue-bound) instead of beside the resize that reads the level, for
    // batches of at least blur_ride_min_images images (smaller batches: whatever the pyramid launches leave unblurred rides).
    // Round 5, 64 pairs: every level riding (0) takes the pyramid's launches from 167 to 99 us and FAST's from 266 to 320 (+ 2 %).
    int blur_ride_from = 0, blur_ride_min_images = 64;
    // Level 0 read in place from the caller's packed CV_8UC1 images (no ingest launch, no copy): possible when level 1 is resized
    // by the LDS-free kernel and nothing stages level 0 through pyr_tail_kernel; ORBFE_NO_INPLACE=1 keeps the copy (A/B, tests).
    // Colour / rectified input always goes through ingest (it computes level 0).
    bool inplace_ok = false;
    // FAST on level 0 needs nothing from the pyramid: for batches of at least fast_split_min_images images (one stream group, no
    // stage profiling) it is launched on the context's side stream beside the pyramid's launches, and the caller's stream runs the
    // other levels' cells after them (orbfe_fast_launches; run_chain).  INT_MAX: never (one level, or ORBFE_FAST_SPLIT=0).
    int fast_split_min_images = 0x7fffffff;
    bool host_trace = false;       // ORBFE_HOST_TRACE: the per-call choices (run_chain) are printed too
};

// The FAST launches of one call.  Not split: out[0] = every cell and the blur tiles of the levels >= blur_first (nlevels: none); returns 1.
// Split: out[0] = level 0's cells, with level 0's blur tiles if side_blur, and out[1] = the other levels' cells with the tiles of the
// levels >= blur_first that out[0] does not carry; returns 2.  A split that would leave either launch without cells is not made.
int orbfe_fast_launches(const DeviceConfig &cfg, bool split, bool side_blur, int blur_first, FastRange out[2]);

struct HostPlan : LaunchPlan {
    DeviceConfig cfg;
    // device tables (DeviceBuffers members of the same names), padded as the kernels read them; tail_plan is empty when the
    // fused tail is not used
    std::vector<uint32_t> rs_tab, rs_blk;
    std::vector<int> tail_plan, pair_plan;
    std::vector<uint32_t> cell_info, cell_aux, fast_lane_tab, bk_tab, bk_off, bk_emap, blur_tile_info;
    std::vector<uint8_t> slot_level;
    std::vector<int16_t> patch_uv;
    std::vector<uint32_t> mom_tab;
};

// Fills *plan for parameters that orbfe_create has validated; ORBFE_OK, or an error code with its message in err.
int orbfe_build_plan(const orbfe_params &p, int max_images, const PlanKnobs &knobs, HostPlan *plan, char *err, size_t err_len);
