// orbfe_api.hip -- host side of the C ABI declared in include/orbfe.h.
//
// Builds the level / cell / quota tables exactly as ORBextractor::ORBextractor and
// ComputePyramid do (reference src/ORBextractor.cc:405-464,921-946), owns the HBM
// buffers of one batch of images, and enqueues the kernels of the stage files (orbfe_pyramid / fast / octree* / describe / stereo .hip).
// There is no CPU compute path here: without a HIP device orbfe_create fails.
#include "../../include/orbfe.h"
#include "orbfe_device.h"
#include "orbfe_host.h"
#include "orbfe_plan.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

// bit_pattern_31_ (src/ORBextractor.cc:145-403, re-emitted by tools/extract_pattern.py): the default of every context's pattern copy
static const int8_t k_bit_pattern_31[1024] = {
#include "orb_pattern_31.inc"
};
#define ORBFE_MAX_GROUPS 8

struct orbfe_context {
    orbfe_params params;
    DeviceConfig cfg;
    DeviceBuffers buf;
    hipStream_t stream = nullptr;
    uint8_t *d_in = nullptr;      // staging for host-image entry points [max_images][w*h]
    float *d_depth_in = nullptr;  // staging for RGB-D depth
    // pinned host staging of the single-frame entry points (lazily allocated): packed input rows, then one block of
    // outputs per call so a frame costs one stream synchronisation instead of one blocking copy per array
    uint8_t *h_in = nullptr;      // [min(max_images,2)][w*h]
    float *h_depth_in = nullptr;  // [w*h]
    uint8_t *h_out = nullptr;     // see HostOut
    uint8_t *d_pack = nullptr;    // device staging of orbfe_fetch_batch_packed (lazily allocated for max_images)
    size_t d_pack_bytes = 0;
    hipEvent_t ev_pack = nullptr; // recorded behind the staging's device-to-host copy: the next packed fetch (whatever its stream) waits for it before it refills d_pack
    bool ev_pack_set = false;
    uint8_t *d_ham = nullptr;     // scratch for orbfe_hamming_matrix
    void *d_und = nullptr;        // scratch for the undistortion entry points
    size_t d_und_bytes = 0;
    size_t d_ham_bytes = 0;
    int last_images = 0;
    unsigned epoch = 0;       // extraction calls enqueued so far (device-resident frame caches key on it)
    std::vector<int> slot_cnt;    // keypoint counts of the slots of call `slot_cnt_epoch` (host copy, filled by the first fetch)
    unsigned slot_cnt_epoch = ~0u;
    LaunchPlan plan;          // the planner's choices (orbfe_plan.h) besides cfg; use_octree3 may be cleared by orbfe_create
    const uint8_t *last_src = nullptr; // images of the latest enqueue when it ran in place (orbfe_fetch_pyramid's level 0), else null
    bool last_src_owned = false;       // ... and they live in the library's own staging (d_in: the host entry points), which outlives the call
    bool input_retained = false;       // orbfe_set_input_retained: the caller keeps the images of an enqueue call valid until its next call
    // stage timing: ring of PROF_RING calls x (ORBFE_NUM_STAGES + 1) events
    bool profiling = false;
    int prof_every = 1;      // record events on every prof_every-th enqueue call only (orbfe_set_profiling_interval)
    unsigned prof_seq = 0;   // enqueue calls seen while profiling
    bool prof_now = false;   // the current call records
    int prof_only = -1; // >= 0: record only the two events around that stage
    std::vector<hipEvent_t> events;
    int prof_calls = 0;      // calls recorded since the last reset
    int prof_stages[64];     // number of stages recorded by each call in the ring
    int prof_groups = 1;
    // Recorded on the stream of every enqueue call when its work has been queued: what "the latest extraction" means to the
    // blocking fetches and to the matchers on the resident frame.  The caller's stream handle itself is NOT kept -- a caller
    // may enqueue, synchronise and destroy its stream before it fetches.
    hipEvent_t ev_latest = nullptr;
    bool latest_foreign = false; // the latest call ran on a caller's stream
    std::recursive_mutex mu;
    // stream groups (orbfe_set_streams)
    int groups = 1;
    hipStream_t gstreams[ORBFE_MAX_GROUPS] = {};
    hipEvent_t ev_fork = nullptr, ev_join[ORBFE_MAX_GROUPS] = {};
    int8_t pattern[1024];     // host copy of DeviceBuffers::pattern
    std::vector<void *> allocs;
    orbfe_match_state *match = nullptr;
    orbfe_bow_state *bow = nullptr;
    orbfe_pose_state *pose = nullptr;
    DevBuf init_scratch, init_sync; // orbfe_enqueue_find_homography_fundamental's per-hypothesis scratch; the synchronous form's arrays
    hipError_t chain_err = hipSuccess; // a launcher's refusal inside run_chain (enqueue_batch reports it)
    char err[512];
};

static thread_local char g_err[512] = "";

static int fail(orbfe_context *ctx, int code, const char *fmt, ...)
{
    char msg[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof(msg), fmt, ap);
    va_end(ap);
    snprintf(g_err, sizeof(g_err), "%s", msg);
    if (ctx) snprintf(ctx->err, sizeof(ctx->err), "%s", msg);
    return code;
}

int orbfe_fail(orbfe_context *ctx, int code, const char *fmt, ...)
{
    char msg[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof(msg), fmt, ap);
    va_end(ap);
    return fail(ctx, code, "%s", msg);
}
orbfe_match_state *orbfe_ctx_match_state(orbfe_context *ctx)
{
    if (!ctx->match) ctx->match = orbfe_match_state_create();
    return ctx->match;
}
hipStream_t orbfe_ctx_stream(orbfe_context *ctx) { return ctx->stream; }
int orbfe_ctx_device(const orbfe_context *ctx) { return ctx->params.device; }
const orbfe_params *orbfe_ctx_params(const orbfe_context *ctx) { return &ctx->params; }
const float *orbfe_ctx_scale_factors(const orbfe_context *ctx) { return ctx->plan.scale; }
const float *orbfe_ctx_inv_sigma2(const orbfe_context *ctx) { return ctx->plan.inv_sigma2; }
const DeviceConfig *orbfe_ctx_config(const orbfe_context *ctx) { return &ctx->cfg; }
const DeviceBuffers *orbfe_ctx_buffers(const orbfe_context *ctx) { return &ctx->buf; }
unsigned orbfe_ctx_epoch(const orbfe_context *ctx) { return ctx->epoch; }
int orbfe_ctx_wait_foreign_stream(orbfe_context *ctx)
{
    if (ctx->latest_foreign && hipStreamWaitEvent(ctx->stream, ctx->ev_latest, 0) != hipSuccess)
        return fail(ctx, ORBFE_ERR_HIP, "hipStreamWaitEvent on the latest extraction failed");
    return ORBFE_OK;
}
// Orders stream `s` after the latest extraction call without a host wait.  The call's own stream handle is not kept (see
// ev_latest), so a caller stream always waits for the event; waiting for an event of the same stream costs nothing on the GPU.
int orbfe_ctx_order_after_extraction(orbfe_context *ctx, hipStream_t s)
{
    if (!ctx->latest_foreign) {
        if (s == ctx->stream || ctx->epoch == 0) return ORBFE_OK;
        if (hipEventRecord(ctx->ev_latest, ctx->stream) != hipSuccess) return fail(ctx, ORBFE_ERR_HIP, "hipEventRecord on the context's stream failed");
    }
    if (hipStreamWaitEvent(s, ctx->ev_latest, 0) != hipSuccess) return fail(ctx, ORBFE_ERR_HIP, "hipStreamWaitEvent on the latest extraction failed");
    return ORBFE_OK;
}
int orbfe_ctx_last_images(const orbfe_context *ctx) { return ctx->last_images; }
std::recursive_mutex &orbfe_ctx_mutex(orbfe_context *ctx) { return ctx->mu; }
// Keypoint count of image slot `slot` of the latest extraction call: from the host copy the frame entry points leave behind,
// else one blocking read of the counters per call (batched calls whose results were not fetched yet).
int orbfe_ctx_slot_count(orbfe_context *ctx, int slot, int *cnt)
{
    if (slot < 0 || slot >= ctx->last_images)
        return fail(ctx, ORBFE_ERR_INVALID, "device slot %d: the latest extraction call filled %d image slots", slot, ctx->last_images);
    if (ctx->slot_cnt_epoch != ctx->epoch || (int)ctx->slot_cnt.size() < ctx->last_images) {
        if (ctx->latest_foreign && hipEventSynchronize(ctx->ev_latest) != hipSuccess) return fail(ctx, ORBFE_ERR_HIP, "hipEventSynchronize failed");
        ctx->slot_cnt.resize(ctx->last_images);
        if (hipMemcpyAsync(ctx->slot_cnt.data(), ctx->buf.kp_cnt, sizeof(int) * ctx->last_images, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipStreamSynchronize(ctx->stream) != hipSuccess)
            return fail(ctx, ORBFE_ERR_HIP, "reading the keypoint counters failed");
        ctx->slot_cnt_epoch = ctx->epoch;
    }
    *cnt = ctx->slot_cnt[slot];
    return ORBFE_OK;
}
orbfe_pose_state *orbfe_ctx_pose_state(orbfe_context *ctx)
{
    if (!ctx->pose) ctx->pose = orbfe_pose_state_create();
    return ctx->pose;
}
orbfe_bow_state *orbfe_ctx_bow_state(orbfe_context *ctx)
{
    if (!ctx->bow) ctx->bow = orbfe_bow_state_create();
    return ctx->bow;
}

#define HIP_TRY(ctx, expr)                                                                      \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) return fail(ctx, ORBFE_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

extern "C" int orbfe_abi_version(void) { return ORBFE_ABI_VERSION; }
#include "build/orbfe_build_id.h" // generated by the Makefile: sha256 over the library's sources and compile flags
#ifdef ORBFE_PROFILE_CUTS
extern "C" const char *orbfe_build_id(void) { return ORBFE_BUILD_ID "+cuts"; }
#else
extern "C" const char *orbfe_build_id(void) { return ORBFE_BUILD_ID; }
#endif
extern "C" const char *orbfe_last_error(const orbfe_context *ctx) { return ctx ? ctx->err : g_err; }

template <typename T>
static int dev_alloc(orbfe_context *ctx, T **p, size_t count)
{
    void *q = nullptr;
    size_t bytes = sizeof(T) * (count ? count : 1);
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) return fail(ctx, ORBFE_ERR_HIP, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
    ctx->allocs.push_back(q);
    *p = (T *)q;
    return ORBFE_OK;
}

// one host-built table of the plan into a device buffer of its own (an empty table -- no tail plan -- stays null)
template <typename D, typename T>
static int upload(orbfe_context *ctx, D **dst, const std::vector<T> &tab, const char *what)
{
    T *d = nullptr;
    if (tab.empty()) return ORBFE_OK;
    if (const int rc = dev_alloc(ctx, &d, tab.size())) return rc;
    *dst = (D *)d;
    return hipMemcpy(d, tab.data(), tab.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess ? ORBFE_OK : fail(ctx, ORBFE_ERR_HIP, "%s upload failed", what);
}

extern "C" int orbfe_create(const orbfe_params *params, orbfe_context **out)
try {
    if (!params || !out) return fail(nullptr, ORBFE_ERR_INVALID, "null argument");
    *out = nullptr;
    const orbfe_params &p = *params;
    if (p.nlevels < 1 || p.nlevels > ORBFE_MAX_LEVELS || p.nfeatures < 1 || !(p.scale_factor > 1.0f) ||
        p.half_patch_size < 1 || p.half_patch_size > 62 || p.edge_threshold < p.half_patch_size + 4 || p.edge_threshold < 19 ||
        p.width < 1 || p.height < 1 || p.max_images < 1 || p.min_th_fast < 1 || p.ini_th_fast < p.min_th_fast ||
        p.ini_th_fast > 254)
        return fail(nullptr, ORBFE_ERR_INVALID, "invalid orbfe_params"); // edge_threshold >= 19: the rotated test pattern reaches 18 px from a keypoint (describe_kernel stages +-18)
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(nullptr, ORBFE_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");
    if (p.device < 0 || p.device >= ndev) return fail(nullptr, ORBFE_ERR_INVALID, "device %d out of range (%d)", p.device, ndev);
    HostPlan P;
    char msg[512] = "";
    if (const int prc = orbfe_build_plan(p, p.max_images, PlanKnobs::from_env(), &P, msg, sizeof(msg))) return fail(nullptr, prc, "%s", msg);
    orbfe_context *ctx = new (std::nothrow) orbfe_context();
    if (!ctx) return fail(nullptr, ORBFE_ERR_INVALID, "out of host memory");
    ctx->err[0] = 0;
    ctx->params = p;
    ctx->cfg = P.cfg;
    ctx->plan = P;
    if (hipSetDevice(p.device) != hipSuccess) { delete ctx; return fail(nullptr, ORBFE_ERR_NO_DEVICE, "hipSetDevice failed"); }
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { delete ctx; return fail(nullptr, ORBFE_ERR_NO_DEVICE, "hipStreamCreate failed"); }
    if (hipEventCreateWithFlags(&ctx->ev_latest, hipEventDisableTiming) != hipSuccess) { orbfe_destroy(ctx); return fail(nullptr, ORBFE_ERR_NO_DEVICE, "hipEventCreate failed"); }
    // the one runtime input of the plan: the LDS attribute of the bucket-pyramid quadtree (else the generic kernel, walking the slots)
    if (ctx->plan.use_octree3 && orbfe_octree3_prepare(ctx->plan.ot3_lds, ctx->plan.ot3_nodes_in_hbm) != 0) {
        ctx->plan.use_octree3 = false; ctx->cfg.proc_order = 0;
        // the generic kernel takes over: its LDS tables may not fit where the bucket-pyramid kernel kept its nodes in HBM
        if (orbfe_octree_lds_bytes(ctx->cfg) > 150 * 1024) { ctx->plan.otg_nodes_in_hbm = true; ctx->plan.otg_scratch_bytes = orbfe_otg_level_off(ctx->cfg, ctx->cfg.nlevels); }
        for (int l = 0; l < ctx->cfg.nlevels; l++) // the planner's bound on the generic kernel (orbfe_plan.cpp)
            if (ctx->cfg.lv[l].cand_cap >= (1 << 24)) { orbfe_destroy(ctx); return fail(nullptr, ORBFE_ERR_UNSUPPORTED, "level %d: the bucket-pyramid quadtree kernel could not be prepared and the generic kernel holds fewer than 2^24 candidates per level", l); }
    }
    if (!ctx->plan.use_octree3 && orbfe_octree_generic_prepare(ctx->cfg, ctx->plan.otg_nodes_in_hbm) != 0) {
        // the LDS tables were refused by the runtime: the HBM instantiation needs no attribute
        ctx->plan.otg_nodes_in_hbm = true; ctx->plan.otg_scratch_bytes = orbfe_otg_level_off(ctx->cfg, ctx->cfg.nlevels);
    }
    const DeviceConfig &c = ctx->cfg;
    const size_t B = (size_t)p.max_images;
    DeviceBuffers &b = ctx->buf;
    KeyPointPOD *kps = nullptr;
    int rc = ORBFE_OK;
    auto A = [&](auto &ptr, size_t count) { if (rc == ORBFE_OK) rc = dev_alloc(ctx, &ptr, count); };
    auto Z = [&](void *ptr, size_t bytes) { if (rc == ORBFE_OK && hipMemset(ptr, 0, bytes) != hipSuccess) rc = fail(ctx, ORBFE_ERR_HIP, "hipMemset failed"); };
    auto T = [&](auto **dst, const auto &tab, const char *what) { if (rc == ORBFE_OK) rc = upload(ctx, dst, tab, what); };
    A(b.pyr, B * c.pyr_bytes);
    A(b.blur, B * c.blur_bytes);
    A(b.cell_cnt, B * c.cells_total);
    A(b.cell_xy, B * c.cells_total * c.cell_cap);
    A(b.cell_sc, B * c.cells_total * c.cell_cap);
    A(b.cell_base, B * c.cells_total);
    A(b.cand_xy, B * c.cand_total);
    A(b.cand_sc, B * c.cand_total);
    A(b.ot_xy2, B * c.cand_total);
    A(b.idx0, B * c.cand_total);
    A(b.idx1, B * c.cand_total);
    A(b.bk_end, B * c.nlevels * 4097);
    if (ctx->plan.use_octree3) A(b.bk_best, B * c.nlevels * ORBFE_BK_PYR);
    if (ctx->plan.use_octree3 && ctx->plan.ot3_nodes_in_hbm) A(b.ot3_scratch, B * c.nlevels * orbfe_octree3_node_bytes(c.max_nodes, ctx->plan.ot_sort_cap));
    if (!ctx->plan.use_octree3 && ctx->plan.otg_nodes_in_hbm) A(b.otg_scratch, B * ctx->plan.otg_scratch_bytes);
    A(b.lvl_ncand, B * c.nlevels); A(b.sel_cnt, B * c.nlevels);
    A(b.sel_xy, B * c.sel_total + 4); // + 4: stereo_rowlist_kernel reads whole quads of slots
    A(b.sel_sc, B * c.sel_total);
    A(b.proc_xy, B * c.sel_total);
    A(b.proc_meta, B * c.sel_total);
    A(kps, B * c.sel_total);
    b.kps = kps;
    A(b.desc, B * c.sel_total * 32);
    A(b.kp_cnt, B);
    A(b.u_right, B * c.sel_total); A(b.depth, B * c.sel_total); A(b.sad, B * c.sel_total);
    A(b.status, B);
    A(ctx->d_in, B * (size_t)p.width * p.height);
    A(b.dbg_ts, 4096);
    const size_t pairs = (B + 1) / 2; // stereo row lists: c.row_cap entries per row of a pair
    A(b.row_cnt, pairs * (size_t)p.height);
    A(b.row_ent, pairs * (size_t)p.height * c.row_cap);
    T(&b.rs_blk, P.rs_blk, "resize block table");
    T(&b.tail_plan, P.tail_plan, "pyramid tail plan");
    T(&b.pair_plan, P.pair_plan, "pyramid pair plan");
    T(&b.rs_tab, P.rs_tab, "resize table");
    T(&b.cell_aux, P.cell_aux, "cell table");
    T(&b.fast_lane_tab, P.fast_lane_tab, "cell table");
    T(&b.cell_info, P.cell_info, "cell table");
    T(&b.bk_tab, P.bk_tab, "bucket table");
    T(&b.bk_off, P.bk_off, "bucket partial table");
    T(&b.bk_emap, P.bk_emap, "bucket partial table");
    A(b.bk_part, B * P.bk_emap.size());
    T(&b.blur_tile_info, P.blur_tile_info, "blur tile table");
    T(&b.slot_level, P.slot_level, "slot table");
    T(&b.patch_uv, P.patch_uv, "patch table");
    T(&b.mom_tab, P.mom_tab, "moment table");
    uint32_t *d_pat = nullptr; // the context's copy of the 256 rBRIEF tests (ORBextractor's member `pattern`, src/ORBextractor.cc:442-444)
    A(d_pat, 256);
    if (rc == ORBFE_OK && hipMemcpy(d_pat, k_bit_pattern_31, 1024, hipMemcpyHostToDevice) != hipSuccess) rc = fail(ctx, ORBFE_ERR_HIP, "pattern upload failed");
    b.pattern = d_pat;
    memcpy(ctx->pattern, k_bit_pattern_31, 1024);
    b.lv0 = b.pyr + c.lv[0].pyr_off; b.lv0_stride = c.pyr_bytes; b.lv0_pitch = c.lv[0].pitch; b.lv0_packed = 0;
    Z(b.proc_xy, B * c.sel_total * sizeof(uint32_t)); Z(b.proc_meta, B * c.sel_total * sizeof(uint32_t));
    Z(b.dbg_ts, 4096 * sizeof(long long)); Z(b.row_cnt, pairs * (size_t)p.height * sizeof(int));
    Z(b.bk_part, B * P.bk_emap.size() * sizeof(uint32_t));
    Z(b.kp_cnt, sizeof(int) * B); Z(b.sel_cnt, sizeof(int) * B * c.nlevels); Z(b.status, sizeof(int) * B);
    if (rc != ORBFE_OK) { orbfe_destroy(ctx); return rc; } // fail() has set the thread's error message
    *out = ctx;
    return ORBFE_OK;
} ORBFE_CATCH(nullptr)

extern "C" void orbfe_destroy(orbfe_context *ctx)
{
    if (!ctx) return;
    if (ctx->stream) { hipStreamSynchronize(ctx->stream); }
    for (void *q : ctx->allocs) hipFree(q);
    for (hipEvent_t e : ctx->events) hipEventDestroy(e);
    for (int g = 0; g < ORBFE_MAX_GROUPS; g++) {
        if (ctx->gstreams[g]) { hipStreamSynchronize(ctx->gstreams[g]); hipStreamDestroy(ctx->gstreams[g]); }
        if (ctx->ev_join[g]) hipEventDestroy(ctx->ev_join[g]);
    }
    if (ctx->ev_fork) hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_latest) hipEventDestroy(ctx->ev_latest);
    if (ctx->ev_pack) { if (ctx->ev_pack_set) hipEventSynchronize(ctx->ev_pack); hipEventDestroy(ctx->ev_pack); }
    if (ctx->match) orbfe_match_state_destroy(ctx->match);
    if (ctx->bow) orbfe_bow_state_destroy(ctx->bow);
    if (ctx->pose) orbfe_pose_state_destroy(ctx->pose);
    if (ctx->d_depth_in) hipFree(ctx->d_depth_in);
    if (ctx->h_in) hipHostFree(ctx->h_in);
    if (ctx->h_depth_in) hipHostFree(ctx->h_depth_in);
    if (ctx->h_out) hipHostFree(ctx->h_out);
    if (ctx->d_ham) hipFree(ctx->d_ham);
    if (ctx->d_pack) hipFree(ctx->d_pack);
    for (int sd = 0; sd < 2; sd++) { if (ctx->cfg.rm_xy[sd]) hipFree((void *)ctx->cfg.rm_xy[sd]); if (ctx->cfg.rm_a[sd]) hipFree((void *)ctx->cfg.rm_a[sd]); }
    if (ctx->d_und) hipFree(ctx->d_und);
    if (ctx->stream) hipStreamDestroy(ctx->stream);
    delete ctx;
}

extern "C" int orbfe_get_camera(const orbfe_context *ctx, float *cam)
try {
    if (!ctx || !cam) return ORBFE_ERR_INVALID;
    cam[0] = ctx->params.fx; cam[1] = ctx->params.fy; cam[2] = ctx->params.cx; cam[3] = ctx->params.cy; cam[4] = ctx->params.bf;
    return ORBFE_OK;
} ORBFE_CATCH(nullptr)

static int wait_latest(orbfe_context *ctx);
// ORBextractor copies bit_pattern_31_ into its member `pattern` (src/ORBextractor.cc:442-444); a deployment that distributes the
// table (one broadcast from rank 0: orbslam2_amd/dist.py) hands it to every context here.  Takes effect for calls enqueued afterwards.
extern "C" int orbfe_set_pattern(orbfe_context *ctx, const int32_t *pattern)
try {
    ORBFE_ENTRY(ctx);
    if (!ctx || !pattern) return fail(ctx, ORBFE_ERR_INVALID, "null argument");
    int8_t pk[1024];
    for (int i = 0; i < 512; i++) {
        const int x = pattern[2 * i], y = pattern[2 * i + 1];
        // describe_kernel stages +-18 px around a keypoint (what edge_threshold >= 19 guarantees inside the level): a rotated
        // test point lands cvRound(r * cos / sin) <= cvRound(r) px away, r^2 = x^2 + y^2; r^2 <= 342 <=> r <= 18.493 rounds to 18
        // (bit_pattern_31_ itself reaches r^2 = 338: the point (13, 13))
        if (x < -18 || x > 18 || y < -18 || y > 18 || x * x + y * y > 342)
            return fail(ctx, ORBFE_ERR_UNSUPPORTED, "pattern point %d = (%d, %d) can rotate to more than 18 px from the keypoint", i, x, y);
        pk[2 * i] = (int8_t)x; pk[2 * i + 1] = (int8_t)y;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->params.device));
    { const int rcw = wait_latest(ctx); if (rcw != ORBFE_OK) return rcw; } // calls already enqueued keep the table they were enqueued with
    HIP_TRY(ctx, hipMemcpy((void *)ctx->buf.pattern, pk, 1024, hipMemcpyHostToDevice));
    memcpy(ctx->pattern, pk, 1024);
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

extern "C" int orbfe_get_pattern(const orbfe_context *ctx, int32_t *pattern)
try {
    if (!ctx || !pattern) return ORBFE_ERR_INVALID;
    for (int i = 0; i < 1024; i++) pattern[i] = ctx->pattern[i];
    return ORBFE_OK;
} ORBFE_CATCH(nullptr)

extern "C" int orbfe_levels(const orbfe_context *ctx) { return ctx ? ctx->cfg.nlevels : ORBFE_ERR_INVALID; }
extern "C" int orbfe_keypoint_capacity(const orbfe_context *ctx) { return ctx ? ctx->cfg.sel_total : ORBFE_ERR_INVALID; }

extern "C" int orbfe_get_tables(const orbfe_context *ctx, float *scale, float *inv_scale, float *sigma2,
                                float *inv_sigma2, int32_t *features_per_level, int32_t *umax)
try {
    if (!ctx) return ORBFE_ERR_INVALID;
    const int n = ctx->cfg.nlevels;
    if (scale) memcpy(scale, ctx->plan.scale, sizeof(float) * n);
    if (inv_scale) memcpy(inv_scale, ctx->plan.inv_scale, sizeof(float) * n);
    if (sigma2) memcpy(sigma2, ctx->plan.sigma2, sizeof(float) * n);
    if (inv_sigma2) memcpy(inv_sigma2, ctx->plan.inv_sigma2, sizeof(float) * n);
    if (features_per_level) memcpy(features_per_level, ctx->plan.feats, sizeof(int32_t) * n);
    if (umax) memcpy(umax, ctx->cfg.umax, sizeof(int32_t) * (ctx->cfg.half_patch + 1));
    return ORBFE_OK;
} ORBFE_CATCH(nullptr)

extern "C" int orbfe_level_size(const orbfe_context *ctx, int level, int *w, int *h)
try {
    if (!ctx || level < 0 || level >= ctx->cfg.nlevels) return ORBFE_ERR_INVALID;
    if (w) *w = ctx->cfg.lv[level].w;
    if (h) *h = ctx->cfg.lv[level].h;
    return ORBFE_OK;
} ORBFE_CATCH(nullptr)

static hipStream_t pick_stream(orbfe_context *ctx, void *stream) { return stream ? (hipStream_t)stream : ctx->stream; }

// The blocking fetch entry points copy on the null stream, which does not wait for the non-blocking streams the
// enqueue calls run on: wait for the stream of the latest enqueue (and the context's own) first.
static int wait_latest(orbfe_context *ctx)
{
    if (ctx->latest_foreign) HIP_TRY(ctx, hipEventSynchronize(ctx->ev_latest));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ORBFE_OK;
}

#define PROF_RING 64
static const char *k_stage_names[ORBFE_NUM_STAGES] = {"ingest", "pyramid", "blur", "fast", "octree", "describe",
                                                      "stereo_match", "stereo_median"};
extern "C" const char *orbfe_stage_name(int stage) { return stage >= 0 && stage < ORBFE_NUM_STAGES ? k_stage_names[stage] : ""; }

extern "C" int orbfe_set_profiling(orbfe_context *ctx, int enabled)
try {
    ORBFE_ENTRY(ctx);
    if (!ctx) return ORBFE_ERR_INVALID;
    if (enabled && ctx->events.empty()) {
        ctx->events.resize((size_t)PROF_RING * ORBFE_MAX_GROUPS * (ORBFE_NUM_STAGES + 1));
        for (auto &e : ctx->events) HIP_TRY(ctx, hipEventCreate(&e));
    }
    if (enabled >= 2 + ORBFE_NUM_STAGES || enabled < 0) return fail(ctx, ORBFE_ERR_INVALID, "profiling mode must be 0, 1 or 2 + stage");
    ctx->profiling = enabled != 0;
    ctx->prof_seq = 0;
    ctx->prof_only = enabled >= 2 ? enabled - 2 : -1;
    ctx->prof_calls = 0;
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

extern "C" int orbfe_set_profiling_interval(orbfe_context *ctx, int every)
try {
    ORBFE_ENTRY(ctx);
    if (!ctx || every < 1) return fail(ctx, ORBFE_ERR_INVALID, "interval must be >= 1");
    ctx->prof_every = every;
    ctx->prof_seq = 0;
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

// record event #idx of the current call for stream group `group` (idx 0 = before the first stage)
static inline void prof_mark(orbfe_context *ctx, int group, int idx, hipStream_t s)
{
    if (!ctx->prof_now) return;
    if (ctx->prof_only >= 0 && idx != ctx->prof_only && idx != ctx->prof_only + 1) {
        ctx->prof_stages[ctx->prof_calls % PROF_RING] = idx;
        return;
    }
    const int slot = ctx->prof_calls % PROF_RING;
    hipEventRecord(ctx->events[((size_t)slot * ORBFE_MAX_GROUPS + group) * (ORBFE_NUM_STAGES + 1) + idx], s);
    ctx->prof_stages[slot] = idx;
}

// Per-stage elapsed ms summed over the recorded calls AND over the stream groups of each call
// (with G groups a stage runs as G launches per call, or 7*G for the pyramid).
extern "C" int orbfe_stage_times(orbfe_context *ctx, float *ms, int *calls, int reset)
try {
    ORBFE_ENTRY(ctx);
    if (!ctx || !ms) return ORBFE_ERR_INVALID;
    for (int i = 0; i < ORBFE_NUM_STAGES; i++) ms[i] = 0.f;
    int n = ctx->prof_calls < PROF_RING ? ctx->prof_calls : PROF_RING;
    if (calls) *calls = n;
    if (n > 0) {
        { const int rcw = wait_latest(ctx); if (rcw != ORBFE_OK) return rcw; }
        for (int c = 0; c < n; c++)
            for (int g = 0; g < ctx->prof_groups; g++) {
                const hipEvent_t *ev = &ctx->events[((size_t)c * ORBFE_MAX_GROUPS + g) * (ORBFE_NUM_STAGES + 1)];
                for (int st = 0; st < ctx->prof_stages[c]; st++) {
                    if (ctx->prof_only >= 0 && st != ctx->prof_only) continue;
                    float t = 0.f;
                    HIP_TRY(ctx, hipEventElapsedTime(&t, ev[st], ev[st + 1]));
                    ms[st] += t;
                }
            }
    }
    if (reset) { ctx->prof_calls = 0; ctx->prof_seq = 0; }
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

// View of the per-image buffers starting at image img0 (kernels index images from 0).
static DeviceBuffers shift_buffers(const DeviceBuffers &b, const DeviceConfig &c, int img0)
{
    DeviceBuffers o = b;
    const size_t i = (size_t)img0;
    o.pyr += i * c.pyr_bytes; o.blur += i * c.blur_bytes;
    o.lv0 = o.pyr + c.lv[0].pyr_off; o.lv0_stride = c.pyr_bytes; o.lv0_pitch = c.lv[0].pitch; o.lv0_packed = 0;
    o.cell_cnt += i * c.cells_total; o.cell_base += i * c.cells_total;
    o.cell_xy += i * c.cells_total * c.cell_cap; o.cell_sc += i * c.cells_total * c.cell_cap;
    o.cand_xy += i * c.cand_total; o.cand_sc += i * c.cand_total;
    o.idx0 += i * c.cand_total; o.idx1 += i * c.cand_total; o.ot_xy2 += i * c.cand_total;
    o.lvl_ncand += i * c.nlevels; o.sel_cnt += i * c.nlevels;
    o.bk_part += i * c.bk_part_total; o.bk_end += i * c.nlevels * 4097;
    if (o.ot3_scratch) o.ot3_scratch += i * c.nlevels * orbfe_octree3_node_bytes(c.max_nodes, orbfe_sort_cap(c.max_nodes));
    if (o.bk_best) o.bk_best += i * c.nlevels * ORBFE_BK_PYR;
    if (o.otg_scratch) o.otg_scratch += i * orbfe_otg_level_off(c, c.nlevels);
    o.sel_xy += i * c.sel_total; o.sel_sc += i * c.sel_total; o.proc_xy += i * c.sel_total; o.proc_meta += i * c.sel_total;
    o.kps = (KeyPointPOD *)o.kps + i * c.sel_total; o.desc += i * c.sel_total * 32;
    o.kp_cnt += i; o.status += i;
    o.u_right += i * c.sel_total; o.depth += i * c.sel_total; o.sad += i * c.sel_total;
    o.row_cnt += (i / 2) * (size_t)c.height; o.row_ent += (i / 2) * (size_t)c.height * c.row_cap;
    return o;
}

static int blur_ride_from_of(const orbfe_context *ctx, int n_images)
{
    if (!ctx->plan.fuse_blur) return ctx->cfg.nlevels;
    return n_images >= ctx->plan.blur_ride_min_images ? (ctx->plan.blur_ride_from < ctx->cfg.nlevels ? ctx->plan.blur_ride_from : ctx->cfg.nlevels) : ORBFE_MAX_LEVELS;
}

// First pyramid level whose Gaussian blur rides in FAST's launch for a batch of n_images images (nlevels: none rides; the value is
// an upper bound for batches below the threshold, whose pyramid launches blur as many levels as they reach): what bench.py
// attributes to the dominant kernel's launch.
extern "C" int orbfe_blur_ride_from(const orbfe_context *ctx, int n_images)
try {
    if (!ctx) return ORBFE_ERR_INVALID;
    const int r = blur_ride_from_of(ctx, n_images);
    return r < ctx->cfg.nlevels ? r : (ctx->plan.fuse_blur && n_images < ctx->plan.blur_ride_min_images ? ctx->cfg.nlevels - 1 : ctx->cfg.nlevels);
} ORBFE_CATCH(nullptr)

// One chain of stages over images [img0, img0 + n_images) on stream s; stereo stages if n_pairs > 0.
static void run_chain(orbfe_context *ctx, const uint8_t *d_images, int img0, int n_images, int n_pairs, hipStream_t s, int group)
{
    const DeviceConfig &cfg = ctx->cfg;
    DeviceBuffers buf = shift_buffers(ctx->buf, cfg, img0);
    const uint8_t *src = d_images + (size_t)img0 * cfg.in_image_bytes;
    prof_mark(ctx, group, 0, s);
    if (ctx->plan.inplace_ok && cfg.in_cn == 1 && !cfg.rm_on) { // level 0 = the caller's images (the first pyramid launch clears the status words)
        buf.lv0 = src; buf.lv0_stride = cfg.in_image_bytes; buf.lv0_pitch = cfg.width; buf.lv0_packed = 1;
    } else {
        orbfe_launch_ingest(cfg, buf, src, n_images, s);
    }
    prof_mark(ctx, group, 1, s);
    // levels >= ride_from are left to FAST's launch (orbfe_context::blur_ride_from); the lower ones are blurred beside the resize
    // that reads them, as far as the pyramid's launches reach
    const int ride_from = blur_ride_from_of(ctx, n_images);
    const int blurred = orbfe_launch_pyramid(cfg, buf, n_images, ctx->plan.fuse_blur, s, ride_from);
    prof_mark(ctx, group, 2, s);
    // the levels still unblurred ride in FAST's launch as the last workgroups of each image's block list: FAST is bound by
    // instruction issue, these waves by memory latency.  ORBFE_NO_FUSE=1 gives every blur a launch of its own
    if (!ctx->plan.fuse_blur) orbfe_launch_blur(cfg, buf, n_images, blurred, s);
    prof_mark(ctx, group, 3, s);
    orbfe_launch_fast(cfg, buf, n_images, ctx->plan.use_octree3, s, ctx->plan.fuse_blur ? blurred : cfg.nlevels);
    prof_mark(ctx, group, 4, s);
    if (ctx->plan.use_octree3) orbfe_launch_octree3(cfg, buf, n_images, ctx->plan.ot_sort_cap, ctx->plan.ot3_lds, ctx->plan.ot3_nodes_in_hbm, s);
    else if (const hipError_t e = orbfe_launch_octree_generic(cfg, buf, n_images, ctx->plan.otg_nodes_in_hbm, s)) ctx->chain_err = e;
#ifdef ORBFE_PROFILE_CUTS
    { // EXPERIMENT: see dbg_sort_sel_kernel (orbfe_describe.hip)
        extern void orbfe_launch_dbg_sort_sel(const DeviceConfig &, const DeviceBuffers &, int, int, hipStream_t);
        static const int dbg_sort = getenv("ORBFE_DBG_SORT_SEL") ? atoi(getenv("ORBFE_DBG_SORT_SEL")) : 0;
        if (dbg_sort) orbfe_launch_dbg_sort_sel(cfg, buf, n_images, dbg_sort, s);
    }
#endif
    prof_mark(ctx, group, 5, s);
    orbfe_launch_describe(cfg, buf, n_images, n_pairs > 0, s);
    prof_mark(ctx, group, 6, s);
    if (n_pairs > 0) {
        if (cfg.half_patch != 15) orbfe_launch_stereo_rowlists(cfg, buf, n_pairs, s); // describe_kernel (the reference's patch size) builds them in its own launch
        orbfe_launch_stereo_match(cfg, buf, n_pairs, s);
        prof_mark(ctx, group, 7, s);
        orbfe_launch_stereo_median(cfg, buf, n_pairs, s);
        prof_mark(ctx, group, 8, s);
    }
}

// Images (or pairs) are independent, so a batch is cut into `groups` contiguous sub-batches whose stage
// chains run on separate streams: the latency / barrier-bound stages of one sub-batch (quadtree,
// describe) overlap the VALU-bound stages of another (FAST).  The caller's stream is the fork/join point.
static int enqueue_batch(orbfe_context *ctx, const uint8_t *d_images, int n_units, int imgs_per_unit, void *stream)
{
    hipStream_t s = pick_stream(ctx, stream);
    HIP_TRY(ctx, hipSetDevice(ctx->params.device));
    ctx->prof_now = ctx->profiling && (ctx->prof_seq++ % (unsigned)ctx->prof_every) == 0;
    const int n_images = n_units * imgs_per_unit;
    int G = ctx->groups < n_units ? ctx->groups : n_units;
    if (G < 1) G = 1;
    if (G == 1) {
        run_chain(ctx, d_images, 0, n_images, imgs_per_unit == 2 ? n_units : 0, s, 0);
    } else {
        HIP_TRY(ctx, hipEventRecord(ctx->ev_fork, s));
        int u0 = 0;
        for (int g = 0; g < G; g++) {
            const int nu = n_units / G + (g < n_units % G ? 1 : 0);
            hipStream_t sg = ctx->gstreams[g];
            HIP_TRY(ctx, hipStreamWaitEvent(sg, ctx->ev_fork, 0));
            run_chain(ctx, d_images, u0 * imgs_per_unit, nu * imgs_per_unit, imgs_per_unit == 2 ? nu : 0, sg, g);
            HIP_TRY(ctx, hipEventRecord(ctx->ev_join[g], sg));
            HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->ev_join[g], 0));
            u0 += nu;
        }
    }
    if (ctx->chain_err != hipSuccess) { const hipError_t e = ctx->chain_err; ctx->chain_err = hipSuccess; return fail(ctx, ORBFE_ERR_HIP, "quadtree launch: %s", hipGetErrorString(e)); }
    HIP_TRY(ctx, hipGetLastError());
    ctx->last_src = (ctx->plan.inplace_ok && ctx->cfg.in_cn == 1 && !ctx->cfg.rm_on) ? d_images : nullptr;
    ctx->last_src_owned = ctx->last_src && ctx->last_src == ctx->d_in;
    ctx->last_images = n_images;
    ctx->epoch++;
    ctx->prof_groups = G;
    ctx->latest_foreign = s != ctx->stream;
    if (ctx->latest_foreign) HIP_TRY(ctx, hipEventRecord(ctx->ev_latest, s));
    if (ctx->prof_now) ctx->prof_calls++;
    return ORBFE_OK;
}

extern "C" int orbfe_quadtree_kernel(const orbfe_context *ctx)
try {
    if (!ctx) return 0;
    return ctx->plan.use_octree3 ? 3 : 1;
} ORBFE_CATCH(nullptr)

extern "C" int orbfe_quadtree_plan(const orbfe_context *ctx)
try {
    if (!ctx) return ORBFE_ERR_INVALID;
    if (ctx->plan.use_octree3) return ctx->plan.ot3_nodes_in_hbm ? 1 : 0;
    return ctx->plan.otg_nodes_in_hbm ? 3 : 2;
} ORBFE_CATCH(nullptr)

extern "C" int orbfe_set_streams(orbfe_context *ctx, int groups)
try {
    ORBFE_ENTRY(ctx);
    if (!ctx || groups < 1 || groups > ORBFE_MAX_GROUPS) return fail(ctx, ORBFE_ERR_INVALID, "groups must be in [1, %d]", ORBFE_MAX_GROUPS);
    if (ctx->profiling) return fail(ctx, ORBFE_ERR_INVALID, "change the stream count before enabling profiling");
    HIP_TRY(ctx, hipSetDevice(ctx->params.device));
    if (!ctx->ev_fork) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
    for (int g = 0; g < groups; g++) {
        if (!ctx->gstreams[g]) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->gstreams[g], hipStreamNonBlocking));
        if (!ctx->ev_join[g]) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_join[g], hipEventDisableTiming));
    }
    ctx->groups = groups;
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

// Level 0 of a batched call on packed grey images is the caller's buffer itself (round 4: no ingest copy).  The kernels need it until
// the call's work has finished; orbfe_fetch_pyramid(level 0) would need it AFTER that, which the library cannot know: it follows the
// pointer only for callers that state here that the images of an enqueue call stay valid (and unchanged) until their next call.
extern "C" int orbfe_set_input_retained(orbfe_context *ctx, int retained)
try {
    ORBFE_ENTRY(ctx);
    if (!ctx) return ORBFE_ERR_INVALID;
    ctx->input_retained = retained != 0;
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

extern "C" int orbfe_enqueue_extract(orbfe_context *ctx, const uint8_t *d_images, int n_images, void *stream)
try {
    ORBFE_ENTRY(ctx);
    if (!ctx || !d_images) return fail(ctx, ORBFE_ERR_INVALID, "null argument");
    if (n_images < 1 || n_images > ctx->params.max_images)
        return fail(ctx, ORBFE_ERR_CAPACITY, "n_images %d outside [1, %d]", n_images, ctx->params.max_images);
    return enqueue_batch(ctx, d_images, n_images, 1, stream);
} ORBFE_CATCH(ctx)

extern "C" int orbfe_enqueue_stereo(orbfe_context *ctx, const uint8_t *d_images, int n_pairs, void *stream)
try {
    ORBFE_ENTRY(ctx);
    if (!ctx || !d_images) return fail(ctx, ORBFE_ERR_INVALID, "null argument");
    if (n_pairs < 1 || 2 * n_pairs > ctx->params.max_images)
        return fail(ctx, ORBFE_ERR_CAPACITY, "n_pairs %d needs max_images >= %d", n_pairs, 2 * n_pairs);
    return enqueue_batch(ctx, d_images, n_pairs, 2, stream);
} ORBFE_CATCH(ctx)

// the staging of the host entry points is sized by the input format: one packed image = image_bytes
static int resize_input_staging(orbfe_context *ctx, size_t image_bytes)
{
    uint8_t *nd = nullptr;
    HIP_TRY(ctx, hipMalloc((void **)&nd, (size_t)ctx->params.max_images * image_bytes));
    for (void *&q : ctx->allocs)
        if (q == ctx->d_in) q = nd;
    (void)hipFree(ctx->d_in);
    if (ctx->last_src == ctx->d_in) ctx->last_src = nullptr; // the latest call's level 0 lived there (orbfe_fetch_pyramid)
    ctx->d_in = nd;
    if (ctx->h_in) { (void)hipHostFree(ctx->h_in); ctx->h_in = nullptr; }
    ctx->cfg.in_image_bytes = image_bytes;
    return ORBFE_OK;
}

extern "C" int orbfe_set_rectification(orbfe_context *ctx, int side, const float *map_x, const float *map_y, int src_w, int src_h)
try {
    ORBFE_ENTRY(ctx);
    if (!ctx || side < 0 || side > 1) return fail(ctx, ORBFE_ERR_INVALID, "bad argument");
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    DeviceConfig &c = ctx->cfg;
    if (!map_x || !map_y) { // clear this side; the left side switches rectification off
        if (c.rm_xy[side]) { (void)hipFree((void *)c.rm_xy[side]); (void)hipFree((void *)c.rm_a[side]); c.rm_xy[side] = nullptr; c.rm_a[side] = nullptr; }
        if (side == 0 && c.rm_on) {
            if (c.rm_xy[1]) { (void)hipFree((void *)c.rm_xy[1]); (void)hipFree((void *)c.rm_a[1]); c.rm_xy[1] = nullptr; c.rm_a[1] = nullptr; }
            c.rm_on = 0;
            return resize_input_staging(ctx, (size_t)ctx->params.width * ctx->params.height * c.in_cn);
        }
        return ORBFE_OK;
    }
    if (c.in_cn != 1) return fail(ctx, ORBFE_ERR_UNSUPPORTED, "rectification takes single-channel input");
    if (src_w < 1 || src_h < 1 || src_w > 32767 || src_h > 32767) return fail(ctx, ORBFE_ERR_INVALID, "bad source size");
    if (side == 1 && !c.rm_on) return fail(ctx, ORBFE_ERR_INVALID, "set the left (side 0) maps first");
    if (c.rm_on && (src_w != c.rm_sw || src_h != c.rm_sh)) {
        if (side == 1 || c.rm_xy[1]) return fail(ctx, ORBFE_ERR_UNSUPPORTED, "both sides must share one source size");
    }
    // RemapInvoker's conversion of the float maps (imgwarp.cpp): sx = cvRound(mapx * INTER_TAB_SIZE), integer part
    // saturated to short, fraction index = (sy & 31) * 32 + (sx & 31)
    const size_t n = (size_t)ctx->params.width * ctx->params.height;
    std::vector<uint32_t> xy(n);
    std::vector<uint16_t> al(n);
    for (size_t i = 0; i < n; i++) {
        const int ix = (int)lrintf(map_x[i] * 32.0f), iy = (int)lrintf(map_y[i] * 32.0f);
        const int sx = std::min(std::max(ix >> 5, -32768), 32767), sy = std::min(std::max(iy >> 5, -32768), 32767);
        xy[i] = (uint32_t)(uint16_t)(int16_t)sx | ((uint32_t)(uint16_t)(int16_t)sy << 16);
        al[i] = (uint16_t)((iy & 31) * 32 + (ix & 31));
    }
    uint32_t *dxy = nullptr; uint16_t *da = nullptr;
    HIP_TRY(ctx, hipMalloc((void **)&dxy, n * sizeof(uint32_t)));
    HIP_TRY(ctx, hipMalloc((void **)&da, n * sizeof(uint16_t)));
    HIP_TRY(ctx, hipMemcpy(dxy, xy.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(da, al.data(), n * sizeof(uint16_t), hipMemcpyHostToDevice));
    if (c.rm_xy[side]) { (void)hipFree((void *)c.rm_xy[side]); (void)hipFree((void *)c.rm_a[side]); }
    c.rm_xy[side] = dxy; c.rm_a[side] = da;
    if (side == 0) {
        c.rm_on = 1; c.rm_sw = src_w; c.rm_sh = src_h;
        return resize_input_staging(ctx, (size_t)src_w * src_h);
    }
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

extern "C" int orbfe_set_input_format(orbfe_context *ctx, int channels, int rgb_order, int legacy_weights)
try {
    ORBFE_ENTRY(ctx);
    if (!ctx) return ORBFE_ERR_INVALID;
    if (channels != 1 && channels != 3 && channels != 4) return fail(ctx, ORBFE_ERR_INVALID, "channels must be 1, 3 or 4");
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->cfg.rm_on && channels != 1) return fail(ctx, ORBFE_ERR_UNSUPPORTED, "rectification takes single-channel input");
    if (channels != ctx->cfg.in_cn) {
        const int rc = resize_input_staging(ctx, (size_t)ctx->params.width * ctx->params.height * channels);
        if (rc != ORBFE_OK) return rc;
    }
    // color_rgb.simd.hpp RGB2Gray<uchar>: RY15 / GY15 / BY15 with 15 fraction bits; OpenCV 3.x: R2Y / G2Y / B2Y with 14
    const int cr = legacy_weights ? 4899 : 9798, cg = legacy_weights ? 9617 : 19235, cb = legacy_weights ? 1868 : 3735;
    ctx->cfg.in_cn = channels;
    ctx->cfg.in_coef[0] = rgb_order ? cr : cb;
    ctx->cfg.in_coef[1] = cg;
    ctx->cfg.in_coef[2] = rgb_order ? cb : cr;
    ctx->cfg.in_shift = legacy_weights ? 14 : 15;
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

extern "C" int orbfe_set_distortion(orbfe_context *ctx, const float *dist, int n)
try {
    ORBFE_ENTRY(ctx);
    if (!ctx || (n != 0 && n != 4 && n != 5) || (n > 0 && !dist)) return fail(ctx, ORBFE_ERR_INVALID, "distortion needs 0, 4 or 5 coefficients (k1 k2 p1 p2 [k3])");
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->cfg.n_dist = n;
    for (int i = 0; i < 5; i++) ctx->cfg.dist[i] = i < n ? dist[i] : 0.f;
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

// scratch for the undistortion entry points: [0, n) input keypoints, [n, 2n) output
static int undistort_on_device(orbfe_context *ctx, const orbfe_keypoint *kps, const KeyPointPOD *d_src, int n, orbfe_keypoint *kps_un)
{
    if (n <= 0) return ORBFE_OK;
    const size_t need = sizeof(KeyPointPOD) * (size_t)n * 2;
    if (ctx->d_und_bytes < need) {
        if (ctx->d_und) (void)hipFree(ctx->d_und);
        ctx->d_und = nullptr; ctx->d_und_bytes = 0;
        HIP_TRY(ctx, hipMalloc((void **)&ctx->d_und, need));
        ctx->d_und_bytes = need;
    }
    KeyPointPOD *d_in = (KeyPointPOD *)ctx->d_und, *d_out = d_in + n;
    if (kps) { HIP_TRY(ctx, hipMemcpyAsync(d_in, kps, sizeof(KeyPointPOD) * n, hipMemcpyHostToDevice, ctx->stream)); d_src = d_in; }
    orbfe_launch_undistort(ctx->cfg, d_src, d_out, n, ctx->stream);
    HIP_TRY(ctx, hipMemcpyAsync(kps_un, d_out, sizeof(KeyPointPOD) * n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ORBFE_OK;
}

extern "C" int orbfe_undistort_keypoints(orbfe_context *ctx, const orbfe_keypoint *kps, int n, orbfe_keypoint *kps_un)
try {
    ORBFE_ENTRY(ctx);
    if (!ctx || n < 0 || (n > 0 && (!kps || !kps_un))) return fail(ctx, ORBFE_ERR_INVALID, "bad argument");
    return undistort_on_device(ctx, kps, nullptr, n, kps_un);
} ORBFE_CATCH(ctx)

extern "C" int orbfe_fetch_keys_un(orbfe_context *ctx, int image, orbfe_keypoint *kps_un, int cap, int *n)
try {
    ORBFE_ENTRY(ctx);
    if (!ctx || image < 0 || image >= ctx->params.max_images || !n) return fail(ctx, ORBFE_ERR_INVALID, "bad argument");
    { const int rcw = wait_latest(ctx); if (rcw != ORBFE_OK) return rcw; }
    int cnt = 0;
    HIP_TRY(ctx, hipMemcpy(&cnt, ctx->buf.kp_cnt + image, sizeof(int), hipMemcpyDeviceToHost));
    *n = cnt;
    if (cnt > cap) return fail(ctx, ORBFE_ERR_CAPACITY, "caller buffer holds %d keypoints, image has %d", cap, cnt);
    if (cnt > 0 && !kps_un) return fail(ctx, ORBFE_ERR_INVALID, "null output");
    return undistort_on_device(ctx, nullptr, (const KeyPointPOD *)ctx->buf.kps + (size_t)image * ctx->cfg.sel_total, cnt, kps_un);
} ORBFE_CATCH(ctx)

extern "C" int orbfe_image_bounds(orbfe_context *ctx, float *bounds)
try {
    ORBFE_ENTRY(ctx);
    if (!ctx || !bounds) return fail(ctx, ORBFE_ERR_INVALID, "bad argument");
    const float cols = (float)ctx->params.width, rows = (float)ctx->params.height;
    if (ctx->cfg.n_dist == 0 || ctx->cfg.dist[0] == 0.0f) { // src/Frame.cc:455-461
        bounds[0] = 0.f; bounds[1] = cols; bounds[2] = 0.f; bounds[3] = rows;
        return ORBFE_OK;
    }
    orbfe_keypoint c[4] = {}, o[4];
    c[1].x = cols; c[2].y = rows; c[3].x = cols; c[3].y = rows; // :439-442
    const int rc = undistort_on_device(ctx, c, nullptr, 4, o);
    if (rc != ORBFE_OK) return rc;
    bounds[0] = std::min(o[0].x, o[2].x);
    bounds[1] = std::max(o[1].x, o[3].x);
    bounds[2] = std::min(o[0].y, o[1].y);
    bounds[3] = std::max(o[2].y, o[3].y);
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

extern "C" int orbfe_synchronize(orbfe_context *ctx, void *stream)
try {
    ORBFE_ENTRY(ctx);
    if (!ctx) return ORBFE_ERR_INVALID;
    HIP_TRY(ctx, hipStreamSynchronize(pick_stream(ctx, stream)));
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

extern "C" int orbfe_fetch_counts(orbfe_context *ctx, int32_t *counts, int n_images)
try {
    ORBFE_ENTRY(ctx);
    if (!ctx || !counts || n_images < 1 || n_images > ctx->params.max_images) return fail(ctx, ORBFE_ERR_INVALID, "bad argument");
    { const int rcw = wait_latest(ctx); if (rcw != ORBFE_OK) return rcw; }
    HIP_TRY(ctx, hipMemcpy(counts, ctx->buf.kp_cnt, sizeof(int32_t) * n_images, hipMemcpyDeviceToHost));
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

extern "C" int orbfe_fetch_batch_async(orbfe_context *ctx, int n_images, orbfe_keypoint *kps, uint8_t *desc, int32_t *counts,
                                       float *u_right, float *depth, void *stream)
try {
    ORBFE_ENTRY(ctx);
    if (!ctx || n_images < 1 || n_images > ctx->params.max_images) return fail(ctx, ORBFE_ERR_INVALID, "bad argument");
    hipStream_t s = pick_stream(ctx, stream);
    const size_t n = (size_t)n_images * ctx->cfg.sel_total;
    if (kps) HIP_TRY(ctx, hipMemcpyAsync(kps, ctx->buf.kps, sizeof(KeyPointPOD) * n, hipMemcpyDeviceToHost, s));
    if (desc) HIP_TRY(ctx, hipMemcpyAsync(desc, ctx->buf.desc, (size_t)32 * n, hipMemcpyDeviceToHost, s));
    if (counts) HIP_TRY(ctx, hipMemcpyAsync(counts, ctx->buf.kp_cnt, sizeof(int32_t) * n_images, hipMemcpyDeviceToHost, s));
    if (u_right) HIP_TRY(ctx, hipMemcpyAsync(u_right, ctx->buf.u_right, sizeof(float) * n, hipMemcpyDeviceToHost, s));
    if (depth) HIP_TRY(ctx, hipMemcpyAsync(depth, ctx->buf.depth, sizeof(float) * n, hipMemcpyDeviceToHost, s));
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

// ---- packed result block (include/orbfe.h: orbfe_packed_layout) ----
static int packed_layout(const orbfe_context *ctx, int n_images, int flags, orbfe_packed_layout *o)
{
    if (!ctx || !o || n_images < 1 || n_images > ctx->params.max_images || (flags & ~(ORBFE_PACK_STEREO | ORBFE_PACK_LEFT_ONLY | ORBFE_PACK_DIRECT)))
        return ORBFE_ERR_INVALID;
    if ((flags & (ORBFE_PACK_STEREO | ORBFE_PACK_LEFT_ONLY)) && (n_images & 1)) return ORBFE_ERR_INVALID; // pairs L0 R0 L1 R1 ...
    const size_t cap = (size_t)ctx->cfg.sel_total, nl = (size_t)ctx->cfg.nlevels;
    const size_t n_out = (flags & ORBFE_PACK_LEFT_ONLY) ? (size_t)n_images / 2 : (size_t)n_images;
    const size_t n_pairs = (flags & ORBFE_PACK_STEREO) ? (size_t)n_images / 2 : 0;
    auto up = [](size_t v) { return (v + 63) & ~(size_t)63; };
    memset(o, 0, sizeof(*o));
    o->n_images_out = (int32_t)n_out; o->capacity = (int32_t)cap; o->nlevels = (int32_t)nl; o->n_pairs = (int32_t)n_pairs; o->flags = flags;
    size_t off = 0;
    o->counts_off = off; off = up(off + 4 * n_out);
    o->level_counts_off = off; off = up(off + 4 * n_out * nl);
    o->xy_off = off; off = up(off + 4 * n_out * cap);
    o->angle_off = off; off = up(off + 4 * n_out * cap);
    o->response_off = off; off = up(off + n_out * cap);
    o->desc_off = off; off = up(off + 32 * n_out * cap);
    o->u_right_off = off; off = up(off + 4 * n_pairs * cap);
    o->depth_off = off; off = up(off + 4 * n_pairs * cap);
    o->bytes = off;
    return ORBFE_OK;
}

extern "C" int orbfe_get_packed_layout(const orbfe_context *ctx, int n_images, int flags, orbfe_packed_layout *out)
try {
    return packed_layout(ctx, n_images, flags, out);
} ORBFE_CATCH(nullptr)

extern "C" int orbfe_fetch_batch_packed(orbfe_context *ctx, int n_images, int flags, void *host_block, size_t host_bytes, void *stream)
try {
    ORBFE_ENTRY(ctx);
    orbfe_packed_layout lay;
    if (packed_layout(ctx, n_images, flags, &lay) != ORBFE_OK || !host_block) return fail(ctx, ORBFE_ERR_INVALID, "bad argument");
    if (n_images > ctx->last_images) return fail(ctx, ORBFE_ERR_INVALID, "the latest extraction call filled %d image slots, %d asked for", ctx->last_images, n_images);
    if (host_bytes < lay.bytes) return fail(ctx, ORBFE_ERR_CAPACITY, "packed block needs %zu bytes, caller offers %zu", lay.bytes, host_bytes);
    HIP_TRY(ctx, hipSetDevice(ctx->params.device));
    PackedOffsets po = {lay.counts_off, lay.level_counts_off, lay.xy_off, lay.angle_off, lay.response_off, lay.desc_off, lay.u_right_off, lay.depth_off};
    if (flags & ORBFE_PACK_DIRECT) {
        // the caller's block is pinned host memory mapped into this device's address space: the gather kernel stores into it
        // across the link itself (posted writes), so no copy engine is involved -- on the measured link an upload and a download
        // queued on the copy engines take the SUM of their times, while a kernel's stores run beside an upload
        {   // checked on every call (a microsecond): the block a caller passes today may not be the pinned one it passed yesterday at the same address
            hipPointerAttribute_t at;
            void *dp = nullptr;
            if (hipPointerGetAttributes(&at, host_block) != hipSuccess || at.type != hipMemoryTypeHost || hipHostGetDevicePointer(&dp, host_block, 0) != hipSuccess || dp != host_block) {
                (void)hipGetLastError();
                return fail(ctx, ORBFE_ERR_INVALID, "ORBFE_PACK_DIRECT needs pinned host memory that the device addresses at the same pointer (hipHostMalloc / hipHostRegister)");
            }
            // ... and the pinned range must hold the whole block: the gather kernel stores lay.bytes from the pointer on
            hipDeviceptr_t base = nullptr;
            size_t range = 0;
            if (hipMemGetAddressRange(&base, &range, (hipDeviceptr_t)host_block) == hipSuccess) {
                if ((const uint8_t *)host_block + lay.bytes > (const uint8_t *)base + range)
                    return fail(ctx, ORBFE_ERR_CAPACITY, "ORBFE_PACK_DIRECT: the pinned range ends %zu bytes after the pointer, the block needs %zu", (size_t)((const uint8_t *)base + range - (const uint8_t *)host_block), lay.bytes);
            } else {
                (void)hipGetLastError(); // the runtime cannot tell (registered memory on some versions): the caller's host_bytes stands
            }
        }
        orbfe_launch_pack_results(ctx->cfg, ctx->buf, (uint8_t *)host_block, po, lay.n_images_out, (flags & ORBFE_PACK_LEFT_ONLY) ? 2 : 1, (flags & ORBFE_PACK_STEREO) != 0, pick_stream(ctx, stream));
        HIP_TRY(ctx, hipGetLastError());
        return ORBFE_OK;
    }
    if (ctx->d_pack_bytes < lay.bytes) { // sized once for the largest block this context can be asked for
        orbfe_packed_layout mx;
        packed_layout(ctx, ctx->params.max_images, 0, &mx); // every image slot, plus uRight / depth of half of them
        const size_t want = mx.bytes + 2 * (((size_t)4 * ((size_t)ctx->params.max_images / 2 + 1) * (size_t)ctx->cfg.sel_total + 63) & ~(size_t)63);
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->ev_pack_set) HIP_TRY(ctx, hipEventSynchronize(ctx->ev_pack)); // a copy out of the old staging may be in flight on a caller's stream
        if (ctx->d_pack) (void)hipFree(ctx->d_pack);
        ctx->d_pack = nullptr; ctx->d_pack_bytes = 0;
        HIP_TRY(ctx, hipMalloc((void **)&ctx->d_pack, want));
        ctx->d_pack_bytes = want;
    }
    hipStream_t s = pick_stream(ctx, stream);
    // ONE staging buffer per context: a fetch queued on another stream while the previous copy is still in flight must not refill it
    if (!ctx->ev_pack) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_pack, hipEventDisableTiming));
    if (ctx->ev_pack_set) HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->ev_pack, 0));
    orbfe_launch_pack_results(ctx->cfg, ctx->buf, ctx->d_pack, po, lay.n_images_out, (flags & ORBFE_PACK_LEFT_ONLY) ? 2 : 1, (flags & ORBFE_PACK_STEREO) != 0, s);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(host_block, ctx->d_pack, lay.bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_pack, s));
    ctx->ev_pack_set = true;
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

// Host side of the packed record: cv::KeyPoint from (level x, level y, octave, score, angle) with the operations of
// src/ORBextractor.cc:838 (size = scaledPatchSize, an int stored as float), :909-915 (pt *= mvScaleFactor[level] for level != 0;
// one IEEE float product each, as describe_kernel's __fmul_rn), cv::KeyPoint's response = (float)score (cv::FAST, :803-808),
// class_id = -1.  Pure host code: no device call, no lock.
extern "C" int orbfe_expand_packed(const orbfe_context *ctx, const void *host_block, const orbfe_packed_layout *lay, int out_image,
                                   orbfe_keypoint *kps, int cap, int *n)
try {
    if (!ctx || !host_block || !lay || !n || out_image < 0 || out_image >= lay->n_images_out || lay->capacity != ctx->cfg.sel_total || lay->nlevels != ctx->cfg.nlevels)
        return ORBFE_ERR_INVALID;
    const uint8_t *b = (const uint8_t *)host_block;
    const int cnt = ((const int32_t *)(b + lay->counts_off))[out_image];
    *n = cnt;
    if (cnt < 0 || cnt > lay->capacity) return ORBFE_ERR_INVALID;
    if (cnt > cap) return ORBFE_ERR_CAPACITY;
    if (cnt > 0 && !kps) return ORBFE_ERR_INVALID;
    const int32_t *lc = (const int32_t *)(b + lay->level_counts_off) + (size_t)out_image * lay->nlevels;
    const uint32_t *xy = (const uint32_t *)(b + lay->xy_off) + (size_t)out_image * lay->capacity;
    const float *ang = (const float *)(b + lay->angle_off) + (size_t)out_image * lay->capacity;
    const uint8_t *rs = b + lay->response_off + (size_t)out_image * lay->capacity;
    int j = 0;
    for (int l = 0; l < lay->nlevels && j < cnt; l++) {
        const float scale = ctx->plan.scale[l], size = (float)ctx->cfg.lv[l].scaled_patch;
        int c = lc[l];
        if (c < 0 || j + c > cnt) return ORBFE_ERR_INVALID;
        for (; c > 0; c--, j++) {
            float px = (float)(xy[j] & 0xffffu), py = (float)(xy[j] >> 16);
            if (l != 0) { px = px * scale; py = py * scale; }
            orbfe_keypoint &k = kps[j];
            k.x = px; k.y = py; k.size = size; k.angle = ang[j]; k.response = (float)rs[j]; k.octave = l; k.class_id = -1;
        }
    }
    return j == cnt ? ORBFE_OK : ORBFE_ERR_INVALID;
} ORBFE_CATCH(nullptr)

extern "C" int orbfe_fetch_image(orbfe_context *ctx, int image, orbfe_keypoint *kps, uint8_t *desc,
                                 float *u_right, float *depth, int cap, int *n)
try {
    ORBFE_ENTRY(ctx);
    if (!ctx || image < 0 || image >= ctx->params.max_images || !n) return fail(ctx, ORBFE_ERR_INVALID, "bad argument");
    { const int rcw = wait_latest(ctx); if (rcw != ORBFE_OK) return rcw; }
    int cnt = 0, status = 0;
    HIP_TRY(ctx, hipMemcpy(&cnt, ctx->buf.kp_cnt + image, sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(&status, ctx->buf.status + image, sizeof(int), hipMemcpyDeviceToHost));
    if (status != 0) return fail(ctx, ORBFE_ERR_CAPACITY, "device-side capacity overflow (status %d) on image %d", status, image);
    *n = cnt;
    if (cnt > cap) return fail(ctx, ORBFE_ERR_CAPACITY, "caller buffers hold %d keypoints, image has %d", cap, cnt);
    const size_t st = (size_t)ctx->cfg.sel_total;
    if (cnt > 0) {
        if (kps) HIP_TRY(ctx, hipMemcpy(kps, (const KeyPointPOD *)ctx->buf.kps + image * st, sizeof(KeyPointPOD) * cnt, hipMemcpyDeviceToHost));
        if (desc) HIP_TRY(ctx, hipMemcpy(desc, ctx->buf.desc + image * st * 32, (size_t)32 * cnt, hipMemcpyDeviceToHost));
        if (u_right) HIP_TRY(ctx, hipMemcpy(u_right, ctx->buf.u_right + image * st, sizeof(float) * cnt, hipMemcpyDeviceToHost));
        if (depth) HIP_TRY(ctx, hipMemcpy(depth, ctx->buf.depth + image * st, sizeof(float) * cnt, hipMemcpyDeviceToHost));
    }
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

extern "C" int orbfe_debug_timestamps(orbfe_context *ctx, long long *dst, int n)
try {
    ORBFE_ENTRY(ctx);
    if (!ctx || !dst || n < 0 || n > 4096) return ORBFE_ERR_INVALID;
    HIP_TRY(ctx, hipMemcpy(dst, ctx->buf.dbg_ts, sizeof(long long) * n, hipMemcpyDeviceToHost));
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

extern "C" int orbfe_device_buffers(orbfe_context *ctx, void **kps, void **desc, void **counts, void **u_right, void **depth)
try {
    ORBFE_ENTRY(ctx);
    if (!ctx) return ORBFE_ERR_INVALID;
    if (kps) *kps = ctx->buf.kps;
    if (desc) *desc = ctx->buf.desc;
    if (counts) *counts = ctx->buf.kp_cnt;
    if (u_right) *u_right = ctx->buf.u_right;
    if (depth) *depth = ctx->buf.depth;
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

// Layout of the pinned output block of the single-frame entry points: counts and status words of the (up to two)
// images, then the keypoint / descriptor / uRight / depth arrays at their device capacity (sel_total per image).
struct HostOut {
    size_t cnt, status, kps, desc, ur, depth, bytes;
};

static HostOut host_out_layout(const orbfe_context *ctx)
{
    const size_t st = (size_t)ctx->cfg.sel_total, ni = ctx->params.max_images < 2 ? 1 : 2;
    HostOut o;
    o.cnt = 0;
    o.status = 16;
    o.kps = 32;
    o.desc = o.kps + ((ni * st * sizeof(KeyPointPOD) + 15) & ~(size_t)15);
    o.ur = o.desc + ni * st * 32;
    o.depth = o.ur + ((st * sizeof(float) + 15) & ~(size_t)15);
    o.bytes = o.depth + st * sizeof(float);
    return o;
}

static int ensure_host_stage(orbfe_context *ctx, bool want_depth)
{
    const size_t px = (size_t)ctx->params.width * ctx->params.height, ni = ctx->params.max_images < 2 ? 1 : 2;
    if (!ctx->h_in) HIP_TRY(ctx, hipHostMalloc((void **)&ctx->h_in, ni * ctx->cfg.in_image_bytes, hipHostMallocDefault));
    if (!ctx->h_out) HIP_TRY(ctx, hipHostMalloc((void **)&ctx->h_out, host_out_layout(ctx).bytes, hipHostMallocDefault));
    if (want_depth && !ctx->h_depth_in) HIP_TRY(ctx, hipHostMalloc((void **)&ctx->h_depth_in, px * sizeof(float), hipHostMallocDefault));
    if (want_depth && !ctx->d_depth_in) HIP_TRY(ctx, hipMalloc((void **)&ctx->d_depth_in, px * sizeof(float)));
    return ORBFE_OK;
}

// Packs the caller's rows into the pinned block and queues one linear copy (a pitched copy from pageable memory is
// executed row by row by the runtime: 3 ms for a 1241x376 image; splitting the copy into chunks to overlap packing
// and DMA costs more in submissions, about 15 us each, than it hides).
static int stage_rows(orbfe_context *ctx, void *d_dst, uint8_t *h_stage, const void *src, size_t row, int h, size_t stride)
{
    if (stride == row) memcpy(h_stage, src, row * h);
    else for (int y = 0; y < h; y++) memcpy(h_stage + (size_t)y * row, (const uint8_t *)src + (size_t)y * stride, row);
    HIP_TRY(ctx, hipMemcpyAsync(d_dst, h_stage, row * h, hipMemcpyHostToDevice, ctx->stream));
    return ORBFE_OK;
}

static int upload_image(orbfe_context *ctx, int slot, const uint8_t *img, int w, int h, size_t stride)
{
    const int ew = ctx->cfg.rm_on ? ctx->cfg.rm_sw : ctx->params.width, eh = ctx->cfg.rm_on ? ctx->cfg.rm_sh : ctx->params.height;
    if (w != ew || h != eh)
        return fail(ctx, ORBFE_ERR_UNSUPPORTED, "image is %dx%d, context expects %dx%d%s", w, h, ew, eh, ctx->cfg.rm_on ? " (unrectified source size)" : "");
    const size_t row = (size_t)w * ctx->cfg.in_cn; // bytes per packed row of the context's input format
    if (stride < row) return fail(ctx, ORBFE_ERR_INVALID, "stride smaller than a row (%d px x %d channels)", w, ctx->cfg.in_cn);
    const size_t px = row * h;
    return stage_rows(ctx, ctx->d_in + (size_t)slot * px, ctx->h_in + (size_t)slot * px, img, row, h, stride);
}

// Queues the device-to-host copies of `nimg` images' results into the pinned block, waits once, and hands the
// caller its arrays.  `with_depth`: image 0 carries uRight / depth.
static int download_frame(orbfe_context *ctx, int nimg, bool with_depth)
{
    const HostOut o = host_out_layout(ctx);
    const size_t st = (size_t)ctx->cfg.sel_total;
    uint8_t *ho = ctx->h_out;
    hipStream_t s = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(ho + o.cnt, ctx->buf.kp_cnt, sizeof(int) * nimg, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(ho + o.status, ctx->buf.status, sizeof(int) * nimg, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(ho + o.kps, ctx->buf.kps, sizeof(KeyPointPOD) * st * nimg, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(ho + o.desc, ctx->buf.desc, (size_t)32 * st * nimg, hipMemcpyDeviceToHost, s));
    if (with_depth) {
        HIP_TRY(ctx, hipMemcpyAsync(ho + o.ur, ctx->buf.u_right, sizeof(float) * st, hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipMemcpyAsync(ho + o.depth, ctx->buf.depth, sizeof(float) * st, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(ctx, hipStreamSynchronize(s));
    ctx->slot_cnt.assign((const int *)(ho + o.cnt), (const int *)(ho + o.cnt) + nimg);
    ctx->slot_cnt_epoch = ctx->epoch;
    return ORBFE_OK;
}

static int hand_over(orbfe_context *ctx, int image, orbfe_keypoint *kps, uint8_t *desc, float *u_right, float *depth,
                     int cap, int *n)
{
    const HostOut o = host_out_layout(ctx);
    const size_t st = (size_t)ctx->cfg.sel_total;
    const uint8_t *ho = ctx->h_out;
    const int cnt = ((const int *)(ho + o.cnt))[image], status = ((const int *)(ho + o.status))[image];
    if (status != 0) return fail(ctx, ORBFE_ERR_CAPACITY, "device-side capacity overflow (status %d) on image %d", status, image);
    *n = cnt;
    if (cnt > cap) return fail(ctx, ORBFE_ERR_CAPACITY, "caller buffers hold %d keypoints, image has %d", cap, cnt);
    if (cnt <= 0) return ORBFE_OK;
    if (kps) memcpy(kps, ho + o.kps + image * st * sizeof(KeyPointPOD), sizeof(KeyPointPOD) * cnt);
    if (desc) memcpy(desc, ho + o.desc + image * st * 32, (size_t)32 * cnt);
    if (u_right) memcpy(u_right, ho + o.ur, sizeof(float) * cnt);
    if (depth) memcpy(depth, ho + o.depth, sizeof(float) * cnt);
    return ORBFE_OK;
}

extern "C" int orbfe_extract(orbfe_context *ctx, const uint8_t *img, int w, int h, size_t stride,
                             orbfe_keypoint *kps, uint8_t *desc, int cap, int *n)
try {
    ORBFE_ENTRY(ctx);
    if (!ctx || !n) return fail(ctx, ORBFE_ERR_INVALID, "null argument");
    if (!img || w <= 0 || h <= 0) { *n = 0; return ORBFE_OK; } // _image.empty(): src/ORBextractor.cc:861-862
    int rc = ensure_host_stage(ctx, false);
    if (rc != ORBFE_OK) return rc;
    rc = upload_image(ctx, 0, img, w, h, stride);
    if (rc != ORBFE_OK) return rc;
    rc = orbfe_enqueue_extract(ctx, ctx->d_in, 1, nullptr);
    if (rc != ORBFE_OK) return rc;
    rc = download_frame(ctx, 1, false);
    if (rc != ORBFE_OK) return rc;
    return hand_over(ctx, 0, kps, desc, nullptr, nullptr, cap, n);
} ORBFE_CATCH(ctx)

extern "C" int orbfe_device_count(void)
try {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
} ORBFE_CATCH(nullptr)

// Host-fed batch in one call: what a single-process multi-device host (orbslam2_amd/host/multi_device.h) runs per context.
extern "C" int orbfe_stereo_batch(orbfe_context *ctx, const uint8_t *images, int n_pairs, orbfe_keypoint *kps, uint8_t *desc, int32_t *counts,
                                  float *u_right, float *depth)
try {
    ORBFE_ENTRY(ctx);
    if (!ctx || !images || !counts) return fail(ctx, ORBFE_ERR_INVALID, "null argument");
    if (n_pairs < 1 || 2 * n_pairs > ctx->params.max_images) return fail(ctx, ORBFE_ERR_CAPACITY, "n_pairs %d needs max_images >= %d", n_pairs, 2 * n_pairs);
    HIP_TRY(ctx, hipSetDevice(ctx->params.device));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_in, images, (size_t)2 * n_pairs * ctx->cfg.in_image_bytes, hipMemcpyHostToDevice, ctx->stream));
    int rc = orbfe_enqueue_stereo(ctx, ctx->d_in, n_pairs, nullptr);
    if (rc != ORBFE_OK) return rc;
    rc = orbfe_fetch_batch_async(ctx, 2 * n_pairs, kps, desc, counts, u_right, depth, nullptr);
    if (rc != ORBFE_OK) return rc;
    // the results are in the caller's buffers once the stream is idle; the status words are read after that, synchronously (an
    // asynchronous copy into a local buffer would outlive it on an early return)
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<int> status((size_t)2 * n_pairs);
    HIP_TRY(ctx, hipMemcpy(status.data(), ctx->buf.status, sizeof(int) * 2 * n_pairs, hipMemcpyDeviceToHost));
    for (int i = 0; i < 2 * n_pairs; i++)
        if (status[i] != 0) return fail(ctx, ORBFE_ERR_CAPACITY, "device-side capacity overflow (status %d) on image %d", status[i], i);
    ctx->slot_cnt.assign(counts, counts + 2 * n_pairs);
    ctx->slot_cnt_epoch = ctx->epoch;
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

// The same batch with the packed result block (one gather kernel + one copy, about two thirds the bytes; orbfe_expand_packed on the host).
extern "C" int orbfe_stereo_batch_packed(orbfe_context *ctx, const uint8_t *images, int n_pairs, int flags, void *host_block, size_t host_bytes)
try {
    ORBFE_ENTRY(ctx);
    if (!ctx || !images || !host_block) return fail(ctx, ORBFE_ERR_INVALID, "null argument");
    if (n_pairs < 1 || 2 * n_pairs > ctx->params.max_images) return fail(ctx, ORBFE_ERR_CAPACITY, "n_pairs %d needs max_images >= %d", n_pairs, 2 * n_pairs);
    HIP_TRY(ctx, hipSetDevice(ctx->params.device));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_in, images, (size_t)2 * n_pairs * ctx->cfg.in_image_bytes, hipMemcpyHostToDevice, ctx->stream));
    int rc = orbfe_enqueue_stereo(ctx, ctx->d_in, n_pairs, nullptr);
    if (rc != ORBFE_OK) return rc;
    rc = orbfe_fetch_batch_packed(ctx, 2 * n_pairs, flags | ORBFE_PACK_STEREO, host_block, host_bytes, nullptr);
    if (rc != ORBFE_OK) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<int> status((size_t)2 * n_pairs);
    HIP_TRY(ctx, hipMemcpy(status.data(), ctx->buf.status, sizeof(int) * 2 * n_pairs, hipMemcpyDeviceToHost));
    for (int i = 0; i < 2 * n_pairs; i++)
        if (status[i] != 0) return fail(ctx, ORBFE_ERR_CAPACITY, "device-side capacity overflow (status %d) on image %d", status[i], i);
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

extern "C" int orbfe_stereo_frame(orbfe_context *ctx, const uint8_t *left, const uint8_t *right,
                                  int w, int h, size_t stride,
                                  orbfe_keypoint *kps_left, uint8_t *desc_left, int *n_left,
                                  orbfe_keypoint *kps_right, uint8_t *desc_right, int *n_right,
                                  float *u_right, float *depth, int cap)
try {
    ORBFE_ENTRY(ctx);
    if (!ctx || !n_left || !n_right) return fail(ctx, ORBFE_ERR_INVALID, "null argument");
    if (!left || !right || w <= 0 || h <= 0) { *n_left = 0; *n_right = 0; return ORBFE_OK; }
    if (ctx->params.max_images < 2) return fail(ctx, ORBFE_ERR_CAPACITY, "stereo needs max_images >= 2");
    int rc = ensure_host_stage(ctx, false);
    if (rc != ORBFE_OK) return rc;
    rc = upload_image(ctx, 0, left, w, h, stride);
    if (rc != ORBFE_OK) return rc;
    rc = upload_image(ctx, 1, right, w, h, stride);
    if (rc != ORBFE_OK) return rc;
    rc = orbfe_enqueue_stereo(ctx, ctx->d_in, 1, nullptr);
    if (rc != ORBFE_OK) return rc;
    rc = download_frame(ctx, 2, true);
    if (rc != ORBFE_OK) return rc;
    rc = hand_over(ctx, 0, kps_left, desc_left, u_right, depth, cap, n_left);
    if (rc != ORBFE_OK) return rc;
    return hand_over(ctx, 1, kps_right, desc_right, nullptr, nullptr, cap, n_right);
} ORBFE_CATCH(ctx)

// Common body of the two RGB-D entry points.  The depth rows are packed while the extraction kernels already run:
// the map is only sampled at the keypoints, at the very end of the chain.
static double host_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static int rgbd_frame_impl(orbfe_context *ctx, const uint8_t *gray, const void *depth_img, size_t px_bytes, float factor,
                           int w, int h, size_t gray_stride, size_t depth_stride,
                           orbfe_keypoint *kps, uint8_t *desc, int *n, float *u_right, float *depth, int cap)
{
    if (!ctx || !n) return fail(ctx, ORBFE_ERR_INVALID, "null argument");
    if (!gray || !depth_img || w <= 0 || h <= 0) { *n = 0; return ORBFE_OK; }
    const size_t row = px_bytes * (size_t)w;
    if (depth_stride < row) return fail(ctx, ORBFE_ERR_INVALID, "depth stride smaller than a row");
    if (ctx->cfg.rm_on) return fail(ctx, ORBFE_ERR_UNSUPPORTED, "RGB-D frames with rectification maps are not supported (the depth map would need the same warp)");
    static const bool trace = getenv("ORBFE_HOST_TRACE") != nullptr;
    double t[6] = {};
    t[0] = host_ms();
    int rc = ensure_host_stage(ctx, true);
    if (rc != ORBFE_OK) return rc;
    rc = upload_image(ctx, 0, gray, w, h, gray_stride);
    if (rc != ORBFE_OK) return rc;
    t[1] = host_ms();
    rc = orbfe_enqueue_extract(ctx, ctx->d_in, 1, nullptr);
    if (rc != ORBFE_OK) return rc;
    t[2] = host_ms();
    rc = stage_rows(ctx, ctx->d_depth_in, (uint8_t *)ctx->h_depth_in, depth_img, row, h, depth_stride);
    if (rc != ORBFE_OK) return rc;
    t[3] = host_ms();
    if (px_bytes == 2) orbfe_launch_rgbd_u16(ctx->cfg, ctx->buf, (const uint16_t *)ctx->d_depth_in, (size_t)w, factor, 0, ctx->stream);
    else orbfe_launch_rgbd(ctx->cfg, ctx->buf, ctx->d_depth_in, (size_t)w, 0, ctx->stream);
    rc = download_frame(ctx, 1, true);
    if (rc != ORBFE_OK) return rc;
    t[4] = host_ms();
    rc = hand_over(ctx, 0, kps, desc, u_right, depth, cap, n);
    t[5] = host_ms();
    if (trace)
        fprintf(stderr, "[orbfe] rgbd frame: gray upload %.3f  enqueue %.3f  depth upload %.3f  rgbd+download+wait %.3f  hand-over %.3f ms\n",
                t[1] - t[0], t[2] - t[1], t[3] - t[2], t[4] - t[3], t[5] - t[4]);
    return rc;
}

extern "C" int orbfe_rgbd_frame(orbfe_context *ctx, const uint8_t *gray, const float *depth_img,
                                int w, int h, size_t gray_stride, size_t depth_stride,
                                orbfe_keypoint *kps, uint8_t *desc, int *n,
                                float *u_right, float *depth, int cap)
try {
    ORBFE_ENTRY(ctx);
    return rgbd_frame_impl(ctx, gray, depth_img, sizeof(float), 1.0f, w, h, gray_stride, depth_stride, kps, desc, n, u_right, depth, cap);
} ORBFE_CATCH(ctx)

extern "C" int orbfe_rgbd_frame_u16(orbfe_context *ctx, const uint8_t *gray, const uint16_t *depth_img, float depth_map_factor,
                                    int w, int h, size_t gray_stride, size_t depth_stride,
                                    orbfe_keypoint *kps, uint8_t *desc, int *n,
                                    float *u_right, float *depth, int cap)
try {
    ORBFE_ENTRY(ctx);
    return rgbd_frame_impl(ctx, gray, depth_img, sizeof(uint16_t), depth_map_factor, w, h, gray_stride, depth_stride, kps, desc, n, u_right, depth, cap);
} ORBFE_CATCH(ctx)

// N RGB-D frames in one chain (BASELINE config 5 batched; the reference builds a multi-camera RGB-D runner, CMakeLists.txt:145-146):
// extraction of the N grey images, then Frame::ComputeStereoFromRGBD (src/Frame.cc:645-666) for every image slot in one launch.
extern "C" int orbfe_enqueue_rgbd(orbfe_context *ctx, const uint8_t *d_gray, const void *d_depth, int depth_is_u16, float depth_map_factor,
                                  int n_images, void *stream)
try {
    ORBFE_ENTRY(ctx);
    if (!ctx || !d_gray || !d_depth) return fail(ctx, ORBFE_ERR_INVALID, "null argument");
    if (n_images < 1 || n_images > ctx->params.max_images) return fail(ctx, ORBFE_ERR_CAPACITY, "n_images %d outside [1, %d]", n_images, ctx->params.max_images);
    if (ctx->cfg.rm_on) return fail(ctx, ORBFE_ERR_UNSUPPORTED, "RGB-D frames with rectification maps are not supported (the depth map would need the same warp)");
    const int rc = enqueue_batch(ctx, d_gray, n_images, 1, stream);
    if (rc != ORBFE_OK) return rc;
    orbfe_launch_rgbd_batch(ctx->cfg, ctx->buf, d_depth, depth_is_u16 != 0, depth_is_u16 ? depth_map_factor : 1.0f, n_images, pick_stream(ctx, stream));
    HIP_TRY(ctx, hipGetLastError());
    if (ctx->latest_foreign) HIP_TRY(ctx, hipEventRecord(ctx->ev_latest, pick_stream(ctx, stream))); // "the latest call" now ends after the depth kernel
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

extern "C" int orbfe_fetch_pyramid(orbfe_context *ctx, int image, int level, int blurred, uint8_t *dst, size_t dst_stride)
try {
    ORBFE_ENTRY(ctx);
    if (!ctx || !dst || image < 0 || image >= ctx->params.max_images || level < 0 || level >= ctx->cfg.nlevels)
        return fail(ctx, ORBFE_ERR_INVALID, "bad argument");
    { const int rcw = wait_latest(ctx); if (rcw != ORBFE_OK) return rcw; }
    const LevelInfo &L = ctx->cfg.lv[level];
    if (dst_stride < (size_t)L.w) return fail(ctx, ORBFE_ERR_INVALID, "dst_stride smaller than level width");
    if (blurred) { // tiled on the device: download the level's tiles and lay the rows out
        const size_t bytes = (size_t)L.blur_tx * ((L.h + 3) / 4) * 128;
        std::vector<uint8_t> t(bytes);
        HIP_TRY(ctx, hipMemcpy(t.data(), ctx->buf.blur + (size_t)image * ctx->cfg.blur_bytes + L.blur_off, bytes, hipMemcpyDeviceToHost));
        for (int y = 0; y < L.h; y++)
            for (int x = 0; x < L.w; x += 4) { // 32 x 4 px tiles of eight 4 x 4 px blocks
                const size_t off = ((size_t)(y >> 2) * L.blur_tx + (x >> 5)) * 128 + (size_t)((x & 31) >> 2) * 16 + (size_t)(y & 3) * 4;
                memcpy(dst + (size_t)y * dst_stride + x, t.data() + off, (size_t)std::min(4, L.w - x));
            }
        return ORBFE_OK;
    }
    if (level == 0 && !blurred && ctx->last_src) { // read in place by the latest call: level 0 IS the caller's image
        // ... which the library does not own: a caller may have freed or reused it once the call's work was done (legal since ABI 1), so
        // the raw pointer is only followed when it is the library's own staging or the caller has promised to keep its images
        if (!ctx->last_src_owned && !ctx->input_retained)
            return fail(ctx, ORBFE_ERR_UNSUPPORTED, "level 0 of the latest call is the caller's own image buffer (read in place, never copied): "
                                                    "call orbfe_set_input_retained(ctx, 1) if that buffer is still valid, or read the images there");
        HIP_TRY(ctx, hipMemcpy2D(dst, dst_stride, ctx->last_src + (size_t)image * ctx->cfg.in_image_bytes, (size_t)L.w, (size_t)L.w, (size_t)L.h, hipMemcpyDeviceToHost));
        return ORBFE_OK;
    }
    const uint8_t *src = ctx->buf.pyr + (size_t)image * ctx->cfg.pyr_bytes + L.pyr_off;
    HIP_TRY(ctx, hipMemcpy2D(dst, dst_stride, src, (size_t)L.pitch, (size_t)L.w, (size_t)L.h, hipMemcpyDeviceToHost));
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

extern "C" int orbfe_fetch_candidates(orbfe_context *ctx, int image, int level, int32_t *xs, int32_t *ys,
                                      int32_t *scores, int cap, int *n)
try {
    ORBFE_ENTRY(ctx);
    if (!ctx || !n || image < 0 || image >= ctx->params.max_images || level < 0 || level >= ctx->cfg.nlevels)
        return fail(ctx, ORBFE_ERR_INVALID, "bad argument");
    { const int rcw = wait_latest(ctx); if (rcw != ORBFE_OK) return rcw; }
    const DeviceConfig &c = ctx->cfg;
    const LevelInfo &L = c.lv[level];
    if (ctx->plan.use_octree3) { // this path never materialises the emission-order arrays; build them for the tap
        orbfe_launch_candidates_gather(c, ctx->buf, ctx->params.max_images, ctx->stream);
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    int nc = 0;
    HIP_TRY(ctx, hipMemcpy(&nc, ctx->buf.lvl_ncand + (size_t)image * c.nlevels + level, sizeof(int), hipMemcpyDeviceToHost));
    *n = nc;
    if (nc > cap) return fail(ctx, ORBFE_ERR_CAPACITY, "caller buffers hold %d candidates, level has %d", cap, nc);
    if (nc == 0) return ORBFE_OK;
    std::vector<uint32_t> xy(nc);
    std::vector<uint8_t> sc(nc);
    HIP_TRY(ctx, hipMemcpy(xy.data(), ctx->buf.cand_xy + (size_t)image * c.cand_total + L.cand_off, sizeof(uint32_t) * nc, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(sc.data(), ctx->buf.cand_sc + (size_t)image * c.cand_total + L.cand_off, (size_t)nc, hipMemcpyDeviceToHost));
    for (int i = 0; i < nc; i++) {
        if (xs) xs[i] = (int32_t)(xy[i] & 0xffffu);
        if (ys) ys[i] = (int32_t)(xy[i] >> 16);
        if (scores) scores[i] = sc[i];
    }
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

extern "C" int orbfe_hamming_matrix(orbfe_context *ctx, const uint8_t *desc_a, int na, const uint8_t *desc_b, int nb, int32_t *dist)
try {
    ORBFE_ENTRY(ctx);
    if (!ctx || !desc_a || !desc_b || !dist || na < 0 || nb < 0) return fail(ctx, ORBFE_ERR_INVALID, "bad argument");
    if (na == 0 || nb == 0) return ORBFE_OK;
    const size_t need = (size_t)32 * na + (size_t)32 * nb + sizeof(int) * (size_t)na * nb;
    if (need > ctx->d_ham_bytes) {
        if (ctx->d_ham) (void)hipFree(ctx->d_ham); // only this entry point's own scratch
        ctx->d_ham = nullptr; ctx->d_ham_bytes = 0;
        HIP_TRY(ctx, hipMalloc((void **)&ctx->d_ham, need));
        ctx->d_ham_bytes = need;
    }
    uint8_t *da = ctx->d_ham, *db = da + (size_t)32 * na;
    int *dd = (int *)(db + (size_t)32 * nb);
    HIP_TRY(ctx, hipMemcpyAsync(da, desc_a, (size_t)32 * na, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(db, desc_b, (size_t)32 * nb, hipMemcpyHostToDevice, ctx->stream));
    orbfe_launch_hamming_matrix(da, na, db, nb, dd, ctx->stream);
    HIP_TRY(ctx, hipMemcpyAsync(dist, dd, sizeof(int) * (size_t)na * nb, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

// The triangulation stage of LocalMapping::CreateNewMapPoints on device-resident keyframes (kernels: orbfe_triangulate_device.hip).
extern "C" int orbfe_enqueue_triangulate_pairs(orbfe_context *ctx, const orbfe_newpoint_keyframe *kf1, const orbfe_newpoint_keyframe *kf2, float mbf,
                                               float ratio_factor, const int32_t *d_pairs, const int32_t *d_npairs, int max_pairs, uint8_t *d_code,
                                               float *d_x3d, int32_t *d_new, int32_t *d_nnew, float *d_pos, int n_rows, int32_t *d_rows_used,
                                               int patch_has_mp, int32_t *d_status, void *stream)
try {
    ORBFE_ENTRY(ctx);
    // what the arguments alone show is refused first, so that the refusals can be told apart without a device
    if (!kf1 || !kf2) return fail(ctx, ORBFE_ERR_INVALID, "triangulate_pairs: null keyframe record");
    if (!d_pairs || !d_npairs) return fail(ctx, ORBFE_ERR_INVALID, "triangulate_pairs: null d_pairs or d_npairs");
    if (!d_code || !d_x3d || !d_new || !d_nnew || !d_status) return fail(ctx, ORBFE_ERR_INVALID, "triangulate_pairs: null output");
    if (kf1->n < 0 || kf2->n < 0 || max_pairs < 0 || n_rows < 0) return fail(ctx, ORBFE_ERR_INVALID, "triangulate_pairs: negative count");
    if (max_pairs > 65535) return fail(ctx, ORBFE_ERR_INVALID, "triangulate_pairs: max_pairs = %d > 65535", max_pairs);
    if (max_pairs > 0)
        for (const orbfe_newpoint_keyframe *kf : {kf1, kf2})
            if (!kf->keys_un || !kf->keys || !kf->u_right || !kf->depth || !kf->cos_stereo || !kf->has_mp)
                return fail(ctx, ORBFE_ERR_INVALID, "triangulate_pairs: null array in a keyframe record");
    if (d_pos && !d_rows_used) return fail(ctx, ORBFE_ERR_INVALID, "triangulate_pairs: d_pos without d_rows_used");
    if (!ctx) return fail(nullptr, ORBFE_ERR_INVALID, "null context");
    orbfe_triangulate_args a;
    a.nlevels = ctx->cfg.nlevels;
    if (a.nlevels < 1 || a.nlevels > ORBFE_MAX_LEVELS) return fail(ctx, ORBFE_ERR_UNSUPPORTED, "nlevels = %d", a.nlevels);
    for (int l = 0; l < ORBFE_MAX_LEVELS; l++) {
        a.scale[l] = l < a.nlevels ? ctx->plan.scale[l] : 1.f;
        a.sigma2[l] = l < a.nlevels ? ctx->plan.sigma2[l] : 1.f;
    }
    a.kf1 = *kf1; a.kf2 = *kf2;
    a.pairs = d_pairs; a.npairs = d_npairs; a.code = d_code; a.x3d = d_x3d; a.new_points = d_new; a.nnew = d_nnew;
    a.pos = d_pos; a.rows_used = d_rows_used; a.status = d_status;
    a.mbf = mbf; a.ratio_factor = ratio_factor;
    a.max_pairs = max_pairs; a.n_rows = n_rows; a.patch_has_mp = patch_has_mp;
    HIP_TRY(ctx, hipSetDevice(ctx->params.device));
    HIP_TRY(ctx, (hipError_t)orbfe_triangulate_launch(a, stream ? (hipStream_t)stream : ctx->stream));
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

// Initializer::FindHomography + FindFundamental for one frame pair (kernels: orbfe_initializer_device.hip).
#include "../host/Initializer.h"
extern "C" int orbfe_enqueue_find_homography_fundamental(orbfe_context *ctx, const orbfe_keypoint *d_keys1_un, int n1, const orbfe_keypoint *d_keys2_un,
                                                         int n2, const int32_t *d_pairs, int N, const int32_t *d_sets, int iterations, const float *norm1,
                                                         const float *norm2, float sigma, float *d_H21, float *d_F21, float *d_score, int32_t *d_best,
                                                         uint8_t *d_inliers_h, uint8_t *d_inliers_f, int32_t *d_ninliers, float *d_all_scores,
                                                         int32_t *d_status, void *stream)
try {
    ORBFE_ENTRY(ctx);
    // what the arguments alone show is refused first, so that the refusals can be told apart without a device
    if (!d_keys1_un || !d_keys2_un || !d_pairs || !d_sets || !norm1 || !norm2) return fail(ctx, ORBFE_ERR_INVALID, "find_homography_fundamental: null input");
    if (!d_H21 || !d_F21 || !d_score || !d_best || !d_status) return fail(ctx, ORBFE_ERR_INVALID, "find_homography_fundamental: null output");
    if (N < 8) return fail(ctx, ORBFE_ERR_INVALID, "find_homography_fundamental: N = %d < 8", N);
    if (iterations < 1) return fail(ctx, ORBFE_ERR_INVALID, "find_homography_fundamental: iterations = %d < 1", iterations);
    if (n1 < 0 || n2 < 0) return fail(ctx, ORBFE_ERR_INVALID, "find_homography_fundamental: negative count");
    if (N > ORBFE_INITIALIZER_MAX_MATCHES || iterations > ORBFE_INITIALIZER_MAX_ITERATIONS || n1 > ORBFE_INITIALIZER_MAX_KEYS || n2 > ORBFE_INITIALIZER_MAX_KEYS)
        return fail(ctx, ORBFE_ERR_INVALID, "find_homography_fundamental: a count above its limit (N %d, iterations %d, n1 %d, n2 %d)", N, iterations, n1, n2);
    if (!(sigma > 0)) return fail(ctx, ORBFE_ERR_INVALID, "find_homography_fundamental: sigma must be > 0");
    if (!ctx) return fail(nullptr, ORBFE_ERR_INVALID, "null context");
    HIP_TRY(ctx, hipSetDevice(ctx->params.device));
    const size_t it = (size_t)iterations;
    if (ctx->init_scratch.ensure(it * (27 + 1 + 2) * 4) != 0) return fail(ctx, ORBFE_ERR_HIP, "find_homography_fundamental: scratch allocation failed");
    orbfe_initializer_args a;
    a.keys1 = d_keys1_un; a.keys2 = d_keys2_un; a.pairs = d_pairs; a.sets = d_sets;
    a.n1 = n1; a.n2 = n2; a.N = N; a.iterations = iterations;
    float T2[9];
    for (int k = 0; k < 4; k++) { a.norm1[k] = norm1[k]; a.norm2[k] = norm2[k]; }
    ORB_SLAM2::InitializerT(a.norm1, a.T1);
    ORB_SLAM2::InitializerT(a.norm2, T2);
    ORB_SLAM2::InitializerInv3(T2, a.T2inv);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) a.T2t[3 * r + c] = T2[3 * c + r];
    a.inv_sigma2 = (float)(1.0 / (double)(sigma * sigma));
    a.H21 = d_H21; a.F21 = d_F21; a.score = d_score; a.best = d_best; a.inl_h = d_inliers_h; a.inl_f = d_inliers_f; a.ninliers = d_ninliers;
    a.all_scores = d_all_scores; a.status = d_status;
    a.mats = (float *)ctx->init_scratch.p; a.ok = (int32_t *)(a.mats + it * 27); a.scores = (float *)(a.ok + it);
    HIP_TRY(ctx, (hipError_t)orbfe_initializer_launch(a, stream ? (hipStream_t)stream : ctx->stream));
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

extern "C" int orbfe_find_homography_fundamental(orbfe_context *ctx, const orbfe_keypoint *keys1_un, int n1, const orbfe_keypoint *keys2_un, int n2,
                                                 const int32_t *matches12, const int32_t *sets, int iterations, float sigma, float *H21, float *F21,
                                                 float *score, int32_t *best, uint8_t *inliers_h, uint8_t *inliers_f, int32_t *ninliers, float *all_scores,
                                                 int32_t *n_matches)
try {
    ORBFE_ENTRY(ctx);
    if (!keys1_un || !keys2_un || !matches12 || !sets) return fail(ctx, ORBFE_ERR_INVALID, "find_homography_fundamental: null input");
    if (!H21 || !F21 || !score || !best || !n_matches) return fail(ctx, ORBFE_ERR_INVALID, "find_homography_fundamental: null output");
    if (n1 < 0 || n2 < 0 || n1 > ORBFE_INITIALIZER_MAX_KEYS || n2 > ORBFE_INITIALIZER_MAX_KEYS || iterations < 1 || iterations > ORBFE_INITIALIZER_MAX_ITERATIONS)
        return fail(ctx, ORBFE_ERR_INVALID, "find_homography_fundamental: a count outside its range (iterations %d, n1 %d, n2 %d)", iterations, n1, n2);
    std::vector<int32_t> pairs; // mvMatches12 (:50-62)
    pairs.reserve(2 * (size_t)n1);
    for (int i = 0; i < n1; i++)
        if (matches12[i] >= 0) { pairs.push_back(i); pairs.push_back(matches12[i]); }
    const int N = (int)(pairs.size() / 2);
    *n_matches = N;
    if (N < 8) return fail(ctx, ORBFE_ERR_INVALID, "find_homography_fundamental: N = %d < 8", N);
    if (N > ORBFE_INITIALIZER_MAX_MATCHES) return fail(ctx, ORBFE_ERR_INVALID, "find_homography_fundamental: N = %d above its limit", N);
    if (!(sigma > 0)) return fail(ctx, ORBFE_ERR_INVALID, "find_homography_fundamental: sigma must be > 0");
    if (!ctx) return fail(nullptr, ORBFE_ERR_INVALID, "null context");
    float norm1[4], norm2[4];
    ORB_SLAM2::NormalizeKeys(keys1_un, n1, norm1);
    ORB_SLAM2::NormalizeKeys(keys2_un, n2, norm2);
    HIP_TRY(ctx, hipSetDevice(ctx->params.device));
    // one device block: inputs, then outputs
    const size_t it = (size_t)iterations, kb1 = sizeof(orbfe_keypoint) * (size_t)n1, kb2 = sizeof(orbfe_keypoint) * (size_t)n2;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 15) & ~(size_t)15; return o; };
    const size_t o_k1 = take(kb1), o_k2 = take(kb2), o_pairs = take(8 * (size_t)N), o_sets = take(32 * it), o_small = take(32 * 4), o_ih = take(N), o_if = take(N),
                 o_all = take(8 * it);
    if (ctx->init_sync.ensure(off) != 0) return fail(ctx, ORBFE_ERR_HIP, "find_homography_fundamental: device allocation failed");
    uint8_t *d = (uint8_t *)ctx->init_sync.p;
    hipStream_t s = ctx->stream;
    if (kb1) HIP_TRY(ctx, hipMemcpyAsync(d + o_k1, keys1_un, kb1, hipMemcpyHostToDevice, s));
    if (kb2) HIP_TRY(ctx, hipMemcpyAsync(d + o_k2, keys2_un, kb2, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(d + o_pairs, pairs.data(), 8 * (size_t)N, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(d + o_sets, sets, 32 * it, hipMemcpyHostToDevice, s));
    // small outputs: H21 [0, 9), F21 [9, 18), score [18, 20), best [20, 22), ninliers [22, 24), status [24]; they start as the caller's H21 / F21
    float small[32] = {};
    memcpy(small, H21, 36); memcpy(small + 9, F21, 36);
    HIP_TRY(ctx, hipMemcpyAsync(d + o_small, small, sizeof(small), hipMemcpyHostToDevice, s));
    float *ds = (float *)(d + o_small);
    const int rc = orbfe_enqueue_find_homography_fundamental(ctx, (const orbfe_keypoint *)(d + o_k1), n1, (const orbfe_keypoint *)(d + o_k2), n2,
                                                             (const int32_t *)(d + o_pairs), N, (const int32_t *)(d + o_sets), iterations, norm1, norm2, sigma, ds,
                                                             ds + 9, ds + 18, (int32_t *)(ds + 20), d + o_ih, d + o_if, (int32_t *)(ds + 22), (float *)(d + o_all),
                                                             (int32_t *)(ds + 24), s);
    if (rc != ORBFE_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(small, d + o_small, sizeof(small), hipMemcpyDeviceToHost, s));
    if (inliers_h) HIP_TRY(ctx, hipMemcpyAsync(inliers_h, d + o_ih, N, hipMemcpyDeviceToHost, s));
    if (inliers_f) HIP_TRY(ctx, hipMemcpyAsync(inliers_f, d + o_if, N, hipMemcpyDeviceToHost, s));
    if (all_scores) HIP_TRY(ctx, hipMemcpyAsync(all_scores, d + o_all, 8 * it, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    memcpy(H21, small, 36); memcpy(F21, small + 9, 36); memcpy(score, small + 18, 8); memcpy(best, small + 20, 8);
    if (ninliers) memcpy(ninliers, small + 22, 8);
    int32_t status;
    memcpy(&status, small + 24, 4);
    if (status != 0) return fail(ctx, status, "find_homography_fundamental: the device reported a faulty pair or set index");
    return ORBFE_OK;
} ORBFE_CATCH(ctx)
