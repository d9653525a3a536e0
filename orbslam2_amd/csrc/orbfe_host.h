// orbfe_host.h -- internal host-side accessors shared by the translation units of liborbfe.so.
#pragma once
#include <hip/hip_runtime.h>
#include <mutex>
#include "../../include/orbfe.h"

// growable device scratch buffer shared by the host-side entry points (matchers, BoW, pose)
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    int ensure(size_t need)
    {
        if (need <= bytes) return 0;
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

struct orbfe_match_state;
orbfe_match_state *orbfe_match_state_create();
void orbfe_match_state_destroy(orbfe_match_state *s);

int orbfe_fail(orbfe_context *ctx, int code, const char *fmt, ...);
// a HIP call inside a function that returns a status: its failure is the context's error, with the call's text
#define ORBFE_HIP_TRY(ctx, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return orbfe_fail(ctx, ORBFE_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); } while (0)
// Every entry point that takes a (non-const) context holds the context's mutex for its whole duration: the reference's
// Tracking, LocalMapping and LoopClosing threads each construct ORBmatcher objects (src/LocalMapping.cc:215,482,
// src/LoopClosing.cc:275,623) and the shim gives them all the left extractor's context, whose matcher / BoW / database state
// (pinned staging, growable device buffers, grid cache, the stream) is single-user.  Recursive: entry points call each other.
std::recursive_mutex &orbfe_ctx_mutex(orbfe_context *ctx);
#define ORBFE_ENTRY(ctx)                                  \
    std::unique_lock<std::recursive_mutex> orbfe_entry_lock_; \
    if (ctx) orbfe_entry_lock_ = std::unique_lock<std::recursive_mutex>(orbfe_ctx_mutex(ctx))
orbfe_match_state *orbfe_ctx_match_state(orbfe_context *ctx);
hipStream_t orbfe_ctx_stream(orbfe_context *ctx);
int orbfe_ctx_device(const orbfe_context *ctx);
const orbfe_params *orbfe_ctx_params(const orbfe_context *ctx);
const float *orbfe_ctx_scale_factors(const orbfe_context *ctx);
// device-resident frames of the latest extraction call (orbfe_match.hip, orbfe_bow.hip)
struct DeviceConfig;
struct DeviceBuffers;
const DeviceConfig *orbfe_ctx_config(const orbfe_context *ctx);
const DeviceBuffers *orbfe_ctx_buffers(const orbfe_context *ctx);
int orbfe_ctx_slot_count(orbfe_context *ctx, int slot, int *cnt); // keypoints in image slot `slot` of the latest extraction call
unsigned orbfe_ctx_epoch(const orbfe_context *ctx);          // counts the extraction calls enqueued on this context
int orbfe_ctx_wait_foreign_stream(orbfe_context *ctx);      // makes the context's stream wait for the latest extraction call (event, no host wait)
int orbfe_ctx_order_after_extraction(orbfe_context *ctx, hipStream_t s); // the same for any stream `s` (the asynchronous matchers run on the caller's)
int orbfe_ctx_last_images(const orbfe_context *ctx);        // image slots the latest extraction call filled

// scratch and caches of the asynchronous, device-resident matchers (orbfe_match_device.hip); owned by orbfe_match_state
struct orbfe_match_device_state;
orbfe_match_device_state *orbfe_ctx_match_device_state(orbfe_context *ctx);
void orbfe_match_device_state_destroy(orbfe_match_device_state *s);

struct orbfe_bow_state;
orbfe_bow_state *orbfe_bow_state_create();
void orbfe_bow_state_destroy(orbfe_bow_state *s);
orbfe_bow_state *orbfe_ctx_bow_state(orbfe_context *ctx);

struct orbfe_pose_state;
orbfe_pose_state *orbfe_pose_state_create();
void orbfe_pose_state_destroy(orbfe_pose_state *s);
orbfe_pose_state *orbfe_ctx_pose_state(orbfe_context *ctx);
const float *orbfe_ctx_inv_sigma2(const orbfe_context *ctx);

// orbfe_enqueue_triangulate_pairs: what the entry point (orbfe_api.hip) hands to the launches (orbfe_triangulate_device.hip); the two
// keyframe records travel by value, the level tables are the context's
#include "orbfe_config.h"
struct orbfe_triangulate_args {
    orbfe_newpoint_keyframe kf1, kf2;
    const int32_t *pairs, *npairs;
    uint8_t *code;
    float *x3d;
    int32_t *new_points, *nnew;
    float *pos;
    int32_t *rows_used, *status;
    float mbf, ratio_factor;
    int max_pairs, n_rows, patch_has_mp, nlevels;
    float scale[ORBFE_MAX_LEVELS], sigma2[ORBFE_MAX_LEVELS]; // mvScaleFactors, mvLevelSigma2
};
int orbfe_triangulate_launch(const orbfe_triangulate_args &a, hipStream_t s); // queues at most three launches; returns hipGetLastError()

// orbfe_enqueue_find_homography_fundamental: what the entry point (orbfe_api.hip) hands to the launches (orbfe_initializer_device.hip).
// T1, T2inv and T2t are made on the host from the two Normalize results; mats, ok and scores are the context's scratch.
struct orbfe_initializer_args {
    const orbfe_keypoint *keys1, *keys2;
    const int32_t *pairs, *sets;
    int n1, n2, N, iterations;
    float norm1[4], norm2[4], T1[9], T2inv[9], T2t[9], inv_sigma2;
    float *H21, *F21, *score;
    int32_t *best;
    uint8_t *inl_h, *inl_f;
    int32_t *ninliers;
    float *all_scores;
    int32_t *status;
    float *mats;     // [iterations][27]: H21i, H12i, F21i
    int32_t *ok;     // [iterations]: the set's eight matches are addressable
    float *scores;   // [2][iterations], as summed (a NaN keeps its bits here)
};
int orbfe_initializer_launch(const orbfe_initializer_args &a, hipStream_t s); // a memset and three launches; returns the first HIP error

// No C++ exception may cross the C ABI (a ctypes / cgo / C caller would abort): every extern "C" function that returns a status is a
// function-try-block closed by this handler.  The per-context lock of ORBFE_ENTRY is a local of the try block, so it is released first.
#include <exception>
#include <new>
#define ORBFE_CATCH(ctxexpr)                                                                                              \
    catch (const std::bad_alloc &) { return orbfe_fail(ctxexpr, ORBFE_ERR_HIP, "out of host memory"); }                   \
    catch (const std::exception &e_) { return orbfe_fail(ctxexpr, ORBFE_ERR_HIP, "host exception: %s", e_.what()); }      \
    catch (...) { return orbfe_fail(ctxexpr, ORBFE_ERR_HIP, "unknown host exception"); }
