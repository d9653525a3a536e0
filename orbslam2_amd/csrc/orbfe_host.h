// orbfe_host.h -- the context and the host-side helpers shared by the translation units of liborbfe.so.
#pragma once
#include <hip/hip_runtime.h>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <vector>
#include "../../include/orbfe.h"
#include "orbfe_arena.hpp"
#include "orbfe_device.h"
#include "orbfe_plan.h"

// growable device scratch buffer shared by the host-side entry points (matchers, BoW, pose)
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    int ensure(size_t need)
    {
        if (need <= bytes) return 0;
        if (need == SIZE_MAX) return -1; // an arena whose size overflowed (orbfe_arena.hpp)
        if (p) (void)hipFree(p);
        p = nullptr; bytes = 0;
        if (hipMalloc(&p, need) != hipSuccess) return -1;
        bytes = need;
        return 0;
    }
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
};

// The staging block of a synchronous entry point: a layout (orbfe_arena.hpp) bound to a device buffer that already holds
// layout.bytes() and to its host image -- the block's own zeroed memory, or the caller's pinned block of at least that size.  One
// copy up, the enqueue form on dev() pointers, one copy of the results down.
class StageBlock {
public:
    StageBlock(const orbfe::StageLayout &layout, const DevBuf &dev, uint8_t *pinned = nullptr) : l_(layout), d_((uint8_t *)dev.p), h_(pinned)
    {
        if (!h_) { own_.assign(l_.bytes(), 0); h_ = own_.data(); }
    }
    template <class T> T *host(orbfe::Field<T> f) const { return (T *)(h_ + f.offset); }
    template <class T> T *dev(orbfe::Field<T> f) const { return (T *)(d_ + f.offset); }
    // n elements into / out of the field, from its element `at` on; they must fit the field
    template <class T> void put(orbfe::Field<T> f, const void *src, size_t n, size_t at = 0) { if (fits(n, at, f.count)) memcpy(host(f) + at, src, sizeof(T) * n); }
    template <class T> void get(orbfe::Field<T> f, void *dst, size_t n, size_t at = 0) const { if (fits(n, at, f.count)) memcpy(dst, host(f) + at, sizeof(T) * n); }
    hipError_t upload(hipStream_t s) const { return hipMemcpyAsync(d_, h_, l_.bytes(), hipMemcpyHostToDevice, s); }
    hipError_t download(hipStream_t s) const { return hipMemcpyAsync(h_, d_, l_.down(), hipMemcpyDeviceToHost, s); }

private:
    static bool fits(size_t n, size_t at, size_t count)
    {
        if (at > count || n > count - at) throw std::length_error("staging block: more elements than the field holds");
        return n > 0;
    }
    const orbfe::StageLayout &l_;
    uint8_t *d_, *h_;
    std::vector<uint8_t> own_;
};

// lazily created state of the feature files; each is destroyed by orbfe_destroy
struct orbfe_match_state;        // orbfe_match.hip
orbfe_match_state *orbfe_match_state_create();
void orbfe_match_state_destroy(orbfe_match_state *s);
struct orbfe_match_device_state; // scratch and caches of the asynchronous, device-resident matchers (orbfe_match_device.hip)
void orbfe_match_device_state_destroy(orbfe_match_device_state *s);
struct orbfe_bow_state;          // orbfe_bow.hip, orbfe_bow_device.hip
orbfe_bow_state *orbfe_bow_state_create();
void orbfe_bow_state_destroy(orbfe_bow_state *s);
struct orbfe_pose_state;         // orbfe_pose.hip
orbfe_pose_state *orbfe_pose_state_create();
void orbfe_pose_state_destroy(orbfe_pose_state *s);

#define ORBFE_MAX_GROUPS 8

struct orbfe_context {
    orbfe_params params;
    DeviceConfig cfg;
    DeviceBuffers buf;        // device-resident frames of the latest extraction call
    hipStream_t stream = nullptr;
    uint8_t *d_in = nullptr;      // staging for host-image entry points [max_images][w*h]
    float *d_depth_in = nullptr;  // staging for RGB-D depth
    // pinned host staging of the single-frame entry points (lazily allocated): packed input rows, then one block of
    // outputs per call so a frame costs one stream synchronisation instead of one blocking copy per array
    uint8_t *h_in = nullptr;      // [min(max_images,2)][w*h]
    float *h_depth_in = nullptr;  // [w*h]
    uint8_t *h_out = nullptr;     // see HostOut
    DevBuf d_pack;                // device staging of orbfe_fetch_batch_packed (lazily allocated for max_images)
    hipEvent_t ev_pack = nullptr; // recorded behind the staging's device-to-host copy: the next packed fetch (whatever its stream) waits for it before it refills d_pack
    bool ev_pack_set = false;
    DevBuf d_ham;                 // scratch for orbfe_hamming_matrix
    DevBuf d_und;                 // scratch for the undistortion entry points
    int last_images = 0;      // image slots the latest extraction call filled
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
    // FAST's level 0 beside the pyramid's launches (run_chain; LaunchPlan::fast_split_min_images): created on first use
    hipStream_t side_stream = nullptr;
    hipEvent_t ev_side_fork = nullptr, ev_side_join = nullptr;
    int fast_split_traced = -1; // the choice ORBFE_HOST_TRACE printed last (0 single, 1 split)
    int8_t pattern[1024];     // host copy of DeviceBuffers::pattern
    std::vector<void *> allocs;
    orbfe_match_state *match = nullptr;
    orbfe_match_device_state *match_device = nullptr;
    orbfe_bow_state *bow = nullptr;
    orbfe_pose_state *pose = nullptr;
    // The scratch of the enqueue forms: one buffer each, so that growing one never frees what the call before it still reads.
    DevBuf init_scratch;        // orbfe_enqueue_find_homography_fundamental's per-hypothesis scratch
    DevBuf recon_scratch;       // the same of orbfe_enqueue_reconstruct_initial
    DevBuf sim3_opt_scratch;    // orbfe_enqueue_optimize_sim3's correspondence table when it does not fit the LDS
    DevBuf sim3_ransac_scratch; // orbfe_enqueue_sim3_ransac_batch's correspondence tables
    DevBuf pnp_ransac_scratch;  // orbfe_enqueue_pnp_ransac_batch's correspondence tables
    DevBuf lba_scratch;         // orbfe_enqueue_local_bundle_adjustment's vertices, per-edge blocks and (above ORBFE_LBA_LDS_KEYFRAMES) reduced system
    DevBuf eg_scratch;          // orbfe_enqueue_optimize_essential_graph's vertices, per-edge blocks, H and (above ORBFE_EG_LDS_DOUBLES) the factorisation's workspace
    // The arrays of the synchronous forms of all seven: each holds the context's mutex, stages into this buffer, and synchronises its
    // stream before it returns, and none calls another, so no two blocks are ever live together.  (PoseOptimization and the
    // matchers keep blocks of their own in their state.)
    DevBuf sync_stage;
    hipError_t chain_err = hipSuccess; // a launcher's refusal inside run_chain (enqueue_batch reports it)
    char err[512];
};

int orbfe_fail(orbfe_context *ctx, int code, const char *fmt, ...);
// a HIP call inside a function that returns a status: its failure is the context's error, with the call's text
#define ORBFE_HIP_TRY(ctx, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return orbfe_fail(ctx, ORBFE_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); } while (0)
// Every entry point that takes a (non-const) context holds the context's mutex for its whole duration: the reference's
// Tracking, LocalMapping and LoopClosing threads each construct ORBmatcher objects (src/LocalMapping.cc:215,482,
// src/LoopClosing.cc:275,623) and the shim gives them all the left extractor's context, whose matcher / BoW / database state
// (pinned staging, growable device buffers, grid cache, the stream) is single-user.  Recursive: entry points call each other.
#define ORBFE_ENTRY(ctx)                                  \
    std::unique_lock<std::recursive_mutex> orbfe_entry_lock_; \
    if (ctx) orbfe_entry_lock_ = std::unique_lock<std::recursive_mutex>((ctx)->mu)

int orbfe_ctx_slot_count(orbfe_context *ctx, int slot, int *cnt); // keypoints in image slot `slot` of the latest extraction call
int orbfe_ctx_wait_foreign_stream(orbfe_context *ctx);      // makes the context's stream wait for the latest extraction call (event, no host wait)
int orbfe_ctx_order_after_extraction(orbfe_context *ctx, hipStream_t s); // the same for any stream `s` (the asynchronous matchers run on the caller's)
// The prologue of an enqueue entry point, after its argument checks: *s = the caller's stream or else the context's, the context's
// device selected and, with after_extraction, *s ordered behind the latest extraction call.
int orbfe_enqueue_on(orbfe_context *ctx, void *stream, bool after_extraction, hipStream_t *s);
orbfe_match_state *orbfe_ctx_match_state(orbfe_context *ctx);
orbfe_match_device_state *orbfe_ctx_match_device_state(orbfe_context *ctx);
orbfe_bow_state *orbfe_ctx_bow_state(orbfe_context *ctx);
orbfe_pose_state *orbfe_ctx_pose_state(orbfe_context *ctx);

// No C++ exception may cross the C ABI (a ctypes / cgo / C caller would abort): every extern "C" function that returns a status is a
// function-try-block closed by this handler.  The per-context lock of ORBFE_ENTRY is a local of the try block, so it is released first.
#include <exception>
#include <new>
#define ORBFE_CATCH(ctxexpr)                                                                                              \
    catch (const std::bad_alloc &) { return orbfe_fail(ctxexpr, ORBFE_ERR_HIP, "out of host memory"); }                   \
    catch (const std::exception &e_) { return orbfe_fail(ctxexpr, ORBFE_ERR_HIP, "host exception: %s", e_.what()); }      \
    catch (...) { return orbfe_fail(ctxexpr, ORBFE_ERR_HIP, "unknown host exception"); }
