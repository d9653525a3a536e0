// orbfe_triangulate_device.hip -- the triangulation stage of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:286-450, with
// KeyFrame::UnprojectStereo, src/KeyFrame.cc:609-625) for the pairs that orbfe_enqueue_search_for_triangulation left in HBM, asynchronous on
// the caller's stream.  The entry point and its checks are at the end of this file; the arithmetic contract is stated in include/orbfe.h and
// DESIGN.md section 4k, and this file, orbslam2_amd/host/Triangulate.h and tests/triangulate_model.py follow it operation by operation.
//
//   triangulate_reset_kernel    status = 0 (and the count of new points when there is nothing else to queue)
//   triangulate_kernel          one lane per pair, 256-thread workgroups.  The work of a pair is one dependent chain (the Jacobi rotations) and
//                               a call has 100 to 600 pairs, so the kernel is latency-bound on a handful of waves; a lane group per pair would
//                               change the order of the double sums, which the contract fixes.  At, Vt and W live in registers: the six (i, j)
//                               rotations are instantiated with static indices and the selection sort carries values, not indices.
//   triangulate_append_kernel   one wave replays the codes in pair order: ballot + popcount with a running base gives the k-th created pair
//                               its slot of d_new and its table row; it learns the number of new points BEFORE it writes, so a table without
//                               room is refused whole.  The has_mp bytes are written as 1 only, so two lanes never disagree.
// All stores are plain vector stores.
#include "../../include/orbfe.h"
#include "orbfe_config.h"
#include "orbfe_host.h"
#include "orbfe_cvmat.hpp"
#include "orbfe_jacobi4.hpp"

#include <cfloat>

static_assert(sizeof(orbfe_newpoint_keyframe) == 136, "orbfe_newpoint_keyframe: six pointers, Tcw, Ow, six camera floats, n");

// what every kernel of this file takes; the two keyframe records travel by value, the level tables are the context's
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
typedef orbfe_triangulate_args Args;

__global__ __launch_bounds__(64) void triangulate_reset_kernel(int32_t *status, int32_t *nnew)
{
    if (threadIdx.x == 0) {
        *status = 0;
        if (nnew) *nnew = 0;
    }
}

// KeyFrame::UnprojectStereo(i): i is inside [0, n) and depth[i] > 0, both checked by the caller
__device__ __forceinline__ void unproject_stereo(const orbfe_newpoint_keyframe &kf, int i, float (&X)[3])
{
    const float z = kf.depth[i];
    const float u = kf.keys[i].x, v = kf.keys[i].y;
    const float c[3] = {__fmul_rn(__fmul_rn(__fsub_rn(u, kf.cx), z), kf.invfx), __fmul_rn(__fmul_rn(__fsub_rn(v, kf.cy), z), kf.invfy), z};
    rwc_times(kf.Tcw, c, kf.Ow, X);
}

// the chi-square test of :362-387 / :389-413; mbf is the CURRENT keyframe's for both
__device__ __forceinline__ bool reprojection_fails(const orbfe_newpoint_keyframe &kf, float kx, float ky, float ur, bool stereo, const float (&X)[3], float z,
                                                   float mbf, float sigma2)
{
    const float x = row_dot_plus<0>(kf.Tcw, X), y = row_dot_plus<1>(kf.Tcw, X);
    const float invz = (float)(1.0 / (double)z);
    const float u = __fadd_rn(__fmul_rn(__fmul_rn(kf.fx, x), invz), kf.cx);
    const float v = __fadd_rn(__fmul_rn(__fmul_rn(kf.fy, y), invz), kf.cy);
    const float ex = __fsub_rn(u, kx), ey = __fsub_rn(v, ky);
    float e = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
    if (!stereo) return (double)e > 5.991 * (double)sigma2;
    const float er = __fsub_rn(__fsub_rn(u, __fmul_rn(mbf, invz)), ur);
    e = __fadd_rn(e, __fmul_rn(er, er));
    return (double)e > 7.8 * (double)sigma2;
}

// one iteration of :286-450: the code, and for a created pair (code <= 2) its position
__device__ __forceinline__ int triangulate_pair(const Args &a, int idx1, int idx2, float (&X)[3])
{
    const orbfe_newpoint_keyframe &kf1 = a.kf1, &kf2 = a.kf2;
    if (idx1 < 0 || idx1 >= kf1.n || idx2 < 0 || idx2 >= kf2.n) return 11;
    const orbfe_keypoint *kp1 = kf1.keys_un + idx1, *kp2 = kf2.keys_un + idx2;
    const int o1 = kp1->octave, o2 = kp2->octave;
    if (o1 < 0 || o1 >= a.nlevels || o2 < 0 || o2 >= a.nlevels) return 11;
    const float x1 = kp1->x, y1 = kp1->y, x2 = kp2->x, y2 = kp2->y;
    const float ur1 = kf1.u_right[idx1], ur2 = kf2.u_right[idx2];
    const bool stereo1 = ur1 >= 0, stereo2 = ur2 >= 0;
    if ((stereo1 && !(kf1.depth[idx1] > 0)) || (stereo2 && !(kf2.depth[idx2] > 0))) return 11; // UnprojectStereo would return an empty Mat

    // Check parallax between rays
    const float xn1[3] = {__fmul_rn(__fsub_rn(x1, kf1.cx), kf1.invfx), __fmul_rn(__fsub_rn(y1, kf1.cy), kf1.invfy), 1.f};
    const float xn2[3] = {__fmul_rn(__fsub_rn(x2, kf2.cx), kf2.invfx), __fmul_rn(__fsub_rn(y2, kf2.cy), kf2.invfy), 1.f};
    float ray1[3], ray2[3];
    rwc_times(kf1.Tcw, xn1, nullptr, ray1);
    rwc_times(kf2.Tcw, xn2, nullptr, ray2);
    const double dot = (double)ray1[0] * (double)ray2[0] + (double)ray1[1] * (double)ray2[1] + (double)ray1[2] * (double)ray2[2];
    const float cos_rays = (float)(dot / (norm3(ray1) * norm3(ray2)));
    const float cos_plus = __fadd_rn(cos_rays, 1.f);
    float cos1 = cos_plus, cos2 = cos_plus;
    if (stereo1) cos1 = kf1.cos_stereo[idx1];
    else if (stereo2) cos2 = kf2.cos_stereo[idx2];
    const float cos_stereo = cos2 < cos1 ? cos2 : cos1; // std::min(cos1, cos2)

    int code;
    if (cos_rays < cos_stereo && cos_rays > 0 && (stereo1 || stereo2 || (double)cos_rays < 0.9998)) {
        // Linear Triangulation Method: A.row(r) = xn_c * Tcw.row(2) - Tcw.row(r'), held transposed
        Jacobi m;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            m.At[c][0] = __fsub_rn(__fmul_rn(xn1[0], kf1.Tcw[8 + c]), kf1.Tcw[c]);
            m.At[c][1] = __fsub_rn(__fmul_rn(xn1[1], kf1.Tcw[8 + c]), kf1.Tcw[4 + c]);
            m.At[c][2] = __fsub_rn(__fmul_rn(xn2[0], kf2.Tcw[8 + c]), kf2.Tcw[c]);
            m.At[c][3] = __fsub_rn(__fmul_rn(xn2[1], kf2.Tcw[8 + c]), kf2.Tcw[4 + c]);
        }
        float v[4];
        null_vector(m, v);
        if (v[3] == 0) return 4;
        const float alpha = (float)(1.0 / (double)v[3]); // Mat / float is a scale
        X[0] = __fmul_rn(v[0], alpha); X[1] = __fmul_rn(v[1], alpha); X[2] = __fmul_rn(v[2], alpha);
        code = 0;
    } else if (stereo1 && cos1 < cos2) {
        unproject_stereo(kf1, idx1, X);
        code = 1;
    } else if (stereo2 && cos2 < cos1) {
        unproject_stereo(kf2, idx2, X);
        code = 2;
    } else
        return 3; // No stereo and very low parallax

    // Check triangulation in front of cameras
    const float z1 = row_dot_plus<2>(kf1.Tcw, X);
    if (z1 <= 0) return 5;
    const float z2 = row_dot_plus<2>(kf2.Tcw, X);
    if (z2 <= 0) return 6;
    // Check reprojection error in first keyframe, then in the second
    if (reprojection_fails(kf1, x1, y1, ur1, stereo1, X, z1, a.mbf, a.sigma2[o1])) return 7;
    if (reprojection_fails(kf2, x2, y2, ur2, stereo2, X, z2, a.mbf, a.sigma2[o2])) return 8;
    // Check scale consistency
    const float n1[3] = {__fsub_rn(X[0], kf1.Ow[0]), __fsub_rn(X[1], kf1.Ow[1]), __fsub_rn(X[2], kf1.Ow[2])};
    const float n2[3] = {__fsub_rn(X[0], kf2.Ow[0]), __fsub_rn(X[1], kf2.Ow[1]), __fsub_rn(X[2], kf2.Ow[2])};
    const float dist1 = (float)norm3(n1), dist2 = (float)norm3(n2);
    if (dist1 == 0 || dist2 == 0) return 9;
    const float ratio_dist = __fdiv_rn(dist2, dist1);
    const float ratio_octave = __fdiv_rn(a.scale[o1], a.scale[o2]);
    if (__fmul_rn(ratio_dist, a.ratio_factor) < ratio_octave || ratio_dist > __fmul_rn(ratio_octave, a.ratio_factor)) return 10;
    return code;
}

__global__ __launch_bounds__(256) void triangulate_kernel(Args a)
{
    const int count = *a.npairs;
    if (count < 0 || count > a.max_pairs) { // nothing else is written
        if (blockIdx.x == 0 && threadIdx.x == 0) *a.status = ORBFE_ERR_INVALID;
        return;
    }
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= count) return;
    float X[3] = {0.f, 0.f, 0.f};
    const int code = triangulate_pair(a, a.pairs[2 * q], a.pairs[2 * q + 1], X);
    a.code[q] = (uint8_t)code;
    if (code == 11) *a.status = ORBFE_ERR_INVALID; // every lane that writes writes this value
    if (code <= 2) {
        a.x3d[3 * (size_t)q] = X[0]; a.x3d[3 * (size_t)q + 1] = X[1]; a.x3d[3 * (size_t)q + 2] = X[2];
    }
}

__global__ __launch_bounds__(64) void triangulate_append_kernel(Args a)
{
    const int lane = threadIdx.x;
    const int count = *a.npairs;
    if (count < 0 || count > a.max_pairs) return;
    int nnew = 0;
    for (int base = 0; base < count; base += 64) {
        const int q = base + lane;
        nnew += __popcll(__ballot(q < count && a.code[q] <= 2));
    }
    bool table = a.pos != nullptr, fits = true;
    int base_row = 0;
    if (table) {
        base_row = *a.rows_used; // read by every lane before lane 0 advances it below
        const bool negative = base_row < 0;
        if (negative || (long long)base_row + nnew > a.n_rows) { // the table, the counter and both has_mp arrays stay untouched
            if (lane == 0) *a.status = negative ? ORBFE_ERR_INVALID : ORBFE_ERR_CAPACITY;
            table = fits = false;
        }
    }
    int k0 = 0;
    for (int base = 0; base < count; base += 64) {
        const int q = base + lane;
        const bool created = q < count && a.code[q] <= 2;
        const u64 mask = __ballot(created);
        if (created) {
            const int k = k0 + __popcll(mask & ((1ull << lane) - 1)); // pair order
            const int idx1 = a.pairs[2 * q], idx2 = a.pairs[2 * q + 1];
            const int row = table ? base_row + k : -1;
            a.new_points[3 * (size_t)k] = idx1; a.new_points[3 * (size_t)k + 1] = idx2; a.new_points[3 * (size_t)k + 2] = row;
            if (table) {
                a.pos[3 * (size_t)row] = a.x3d[3 * (size_t)q]; a.pos[3 * (size_t)row + 1] = a.x3d[3 * (size_t)q + 1];
                a.pos[3 * (size_t)row + 2] = a.x3d[3 * (size_t)q + 2];
            }
            if (a.patch_has_mp && fits && idx1 >= 0 && idx1 < a.kf1.n && idx2 >= 0 && idx2 < a.kf2.n) { // AddMapPoint (:439-440)
                a.kf1.has_mp[idx1] = 1;
                a.kf2.has_mp[idx2] = 1;
            }
        }
        k0 += __popcll(mask);
    }
    if (lane == 0) {
        *a.nnew = nnew;
        if (table) *a.rows_used = base_row + nnew;
    }
}

// The triangulation stage of LocalMapping::CreateNewMapPoints on device-resident keyframes: at most three launches.
extern "C" int orbfe_enqueue_triangulate_pairs(orbfe_context *ctx, const orbfe_newpoint_keyframe *kf1, const orbfe_newpoint_keyframe *kf2, float mbf,
                                               float ratio_factor, const int32_t *d_pairs, const int32_t *d_npairs, int max_pairs, uint8_t *d_code,
                                               float *d_x3d, int32_t *d_new, int32_t *d_nnew, float *d_pos, int n_rows, int32_t *d_rows_used,
                                               int patch_has_mp, int32_t *d_status, void *stream)
try {
    ORBFE_ENTRY(ctx);
    // what the arguments alone show is refused first, so that the refusals can be told apart without a device
    if (!kf1 || !kf2) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "triangulate_pairs: null keyframe record");
    if (!d_pairs || !d_npairs) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "triangulate_pairs: null d_pairs or d_npairs");
    if (!d_code || !d_x3d || !d_new || !d_nnew || !d_status) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "triangulate_pairs: null output");
    if (kf1->n < 0 || kf2->n < 0 || max_pairs < 0 || n_rows < 0) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "triangulate_pairs: negative count");
    if (max_pairs > 65535) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "triangulate_pairs: max_pairs = %d > 65535", max_pairs);
    if (max_pairs > 0)
        for (const orbfe_newpoint_keyframe *kf : {kf1, kf2})
            if (!kf->keys_un || !kf->keys || !kf->u_right || !kf->depth || !kf->cos_stereo || !kf->has_mp)
                return orbfe_fail(ctx, ORBFE_ERR_INVALID, "triangulate_pairs: null array in a keyframe record");
    if (d_pos && !d_rows_used) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "triangulate_pairs: d_pos without d_rows_used");
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    Args a;
    a.nlevels = ctx->cfg.nlevels;
    if (a.nlevels < 1 || a.nlevels > ORBFE_MAX_LEVELS) return orbfe_fail(ctx, ORBFE_ERR_UNSUPPORTED, "nlevels = %d", a.nlevels);
    for (int l = 0; l < ORBFE_MAX_LEVELS; l++) {
        a.scale[l] = l < a.nlevels ? ctx->plan.scale[l] : 1.f;
        a.sigma2[l] = l < a.nlevels ? ctx->plan.sigma2[l] : 1.f;
    }
    a.kf1 = *kf1; a.kf2 = *kf2;
    a.pairs = d_pairs; a.npairs = d_npairs; a.code = d_code; a.x3d = d_x3d; a.new_points = d_new; a.nnew = d_nnew;
    a.pos = d_pos; a.rows_used = d_rows_used; a.status = d_status;
    a.mbf = mbf; a.ratio_factor = ratio_factor;
    a.max_pairs = max_pairs; a.n_rows = n_rows; a.patch_has_mp = patch_has_mp;
    hipStream_t s;
    if (const int rc = orbfe_enqueue_on(ctx, stream, false, &s)) return rc;
    hipLaunchKernelGGL(triangulate_reset_kernel, dim3(1), dim3(64), 0, s, a.status, a.max_pairs == 0 ? a.nnew : nullptr);
    if (a.max_pairs > 0) {
        hipLaunchKernelGGL(triangulate_kernel, dim3((a.max_pairs + 255) / 256), dim3(256), 0, s, a);
        hipLaunchKernelGGL(triangulate_append_kernel, dim3(1), dim3(64), 0, s, a);
    }
    ORBFE_HIP_TRY(ctx, hipGetLastError());
    return ORBFE_OK;
} ORBFE_CATCH(ctx)
