// orbfe_match_resolve.h -- the HOST half of the Tracking-thread matchers: the projection of every map point into one window
// query (what each reference loop does before it calls GetFeaturesInArea), Frame::isInFrustum, and the sequentially greedy
// accept rules of ORBmatcher::SearchByProjection (x3) and SearchForInitialization replayed over per-query candidate lists.
//
// Pure C++ (no HIP, no device types) on purpose: liborbfe.so's orbfe_match.hip includes it for the product path, and
// tests/asan/resolve_harness.cpp compiles the very same text for the CPU with -fsanitize=address,undefined (GPU ASan does not
// exist on this pool; the host logic is where the index arithmetic of the matchers lives).
// What a point is projected against is a View (camera, scale factors, image bounds), built by view_of for host and device alike.
// The per-point arithmetic (one map point -> one window query, one isInFrustum record, rot_bin, three_maxima) is marked
// ORBFE_RESOLVE_HD: empty in a plain C++ compile, host + device under hipcc, where orbfe_match_device.hip runs the same
// statements one lane per map point (device code is compiled without FMA contraction and with IEEE divide / sqrt too).
//
// A candidate is one 64-bit key
//      dist << 36 | ix << 30 | iy << 24 | idx << 8 | octave
// so ascending key order == (Hamming distance, Frame::GetFeaturesInArea order: cell x, cell y, insertion = keypoint index):
// "the first minimum found by the reference's loop" is the smallest key, "the second best" the next one.  The device hands
// over, per query, the K smallest keys that survive the STATIC filters (keypoint blocked before the call; mvuRight gate), plus
// how many survived in all; the rules below add the DYNAMIC ones (a keypoint taken by an earlier query) and ask for the full
// list only when the K keys run out -- rare, and exact when it happens.
#pragma once

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/orbfe.h"
#include "orbfe_config.h" // ORBFE_MAX_LEVELS

#ifdef __HIPCC__
#define ORBFE_RESOLVE_HD __attribute__((host, device))
#else
#define ORBFE_RESOLVE_HD
#endif

namespace orbfe_resolve
{

// One window query of the device kernels (query_window / for_each_hit, orbfe_match_window.hpp): what a map point asks of the frame grid
struct MatchQuery { // 32 bytes
    float u, v, r;
    int min_level, max_level;
    float ur, ur_rad; // right-image check (mvuRight), used when flags & 2
    int flags;        // bit0: valid query, bit1: apply the u_right check
};

struct Camera { float fx, fy, cx, cy, bf, mb; };
static inline Camera camera_of(const orbfe_params *P)
{
    Camera c = {P->fx, P->fy, P->cx, P->cy, P->bf, P->fx != 0.f ? P->bf / P->fx : 0.f}; // mb := mbf / fx
    return c;
}
// A view: the camera with the scale pyramid and the image bounds a map point is projected against.  `keyframe`: the bounds are a
// KeyFrame's, which KeyFrame::IsInImage truncates to ints (kf_is_in_image).
// The per-point functions bind the scalars they use to locals at their head: a kernel's view lies in its kernel-argument segment,
// and a read at first use would wait for it in the middle of the function.
struct View {
    Camera C;
    float sf[ORBFE_MAX_LEVELS]; // mvScaleFactors
    int nlevels;
    float log_sf;
    float min_x, max_x, min_y, max_y;
    int keyframe;
};
// scale_factors: the context's mvScaleFactors, nlevels of them.  The levels past nlevels hold 1 and are never read: every octave or
// level is range-tested or clamped to [0, nlevels) before it indexes sf.
static inline View view_of(const orbfe_params *P, const float *scale_factors, float min_x, float max_x, float min_y, float max_y, int keyframe)
{
    View V;
    V.C = camera_of(P);
    for (int l = 0; l < ORBFE_MAX_LEVELS; l++) V.sf[l] = l < P->nlevels ? scale_factors[l] : 1.f;
    V.nlevels = P->nlevels;
    V.log_sf = logf((float)(double)P->scale_factor); // mfLogScaleFactor = log(mfScaleFactor), src/Frame.cc:71
    V.min_x = min_x; V.max_x = max_x; V.min_y = min_y; V.max_y = max_y;
    V.keyframe = keyframe;
    return V;
}

// ---- projection arithmetic of the matchers: the reference's float expressions in its evaluation order (contract Q4: no FMA
// contraction -- this header must be compiled with -ffp-contract=off) ----
// OPENCV-4.5.5-SEMANTICS: cv::Mat R*x+t for 3x3 * 3x1 CV_32F (small-matrix gemm path)
ORBFE_RESOLVE_HD static inline void rt_apply(const float *T, const float *x, float *out)
{
    for (int i = 0; i < 3; i++) {
        const float t = (T[4 * i] * x[0] + T[4 * i + 1] * x[1]) + T[4 * i + 2] * x[2];
        out[i] = t + T[4 * i + 3];
    }
}
ORBFE_RESOLVE_HD static inline void camera_center(const float *T, float *ow) // -Rcw.t()*tcw
{
    for (int i = 0; i < 3; i++) ow[i] = ((-T[i]) * T[3] + (-T[4 + i]) * T[7]) + (-T[8 + i]) * T[11];
}
// deterministic log for MapPoint::PredictScale (contract Q4)
ORBFE_RESOLVE_HD static inline float log_det(float xf)
{
    double x = (double)xf;
    int e;
    double m = frexp(x, &e);
    if (m < 0.70710678118654752440) { m *= 2.0; e -= 1; }
    const double s = (m - 1.0) / (m + 1.0);
    const double z = s * s;
    double p = 1.0 / 27.0;
    for (int k = 25; k >= 3; k -= 2) p = p * z + 1.0 / (double)k;
    p = p * z + 1.0;
    const double LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;
    return (float)((double)e * LN2_HI + (2.0 * s * p + (double)e * LN2_LO));
}
ORBFE_RESOLVE_HD static inline int predict_scale(float max_distance, float current_dist, float log_sf, int n_levels) // src/MapPoint.cc:402-417
{
    const float ratio = max_distance / current_dist;
    int n_scale = (int)ceilf(log_det(ratio) / log_sf);
    if (n_scale < 0) n_scale = 0;
    else if (n_scale >= n_levels) n_scale = n_levels - 1;
    return n_scale;
}
ORBFE_RESOLVE_HD static inline float norm3(const float *po) { return (float)sqrt((double)po[0] * po[0] + (double)po[1] * po[1] + (double)po[2] * po[2]); }

// ---- one window query per map point: the part of each matcher's loop body that precedes GetFeaturesInArea ----
static const MatchQuery NO_QUERY = {0, 0, 0, 0, -1, 0, 0, 0};

// ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono), src/ORBmatcher.cc:1335-1390.
// The motion test of :1347-1352 (the same for every point) ...
ORBFE_RESOLVE_HD static inline void last_motion(const Camera &C, const float *Tcw_cur, const float *Tcw_last, int mono, bool &forward, bool &backward)
{
    float twc[3], tlc[3];
    camera_center(Tcw_cur, twc);
    rt_apply(Tcw_last, twc, tlc);
    forward = tlc[2] > C.mb && !mono;
    backward = -tlc[2] > C.mb && !mono;
}
// ... and the loop body for one map point of the last frame.  Q must hold NO_QUERY; returns -1 on a bad octave.
ORBFE_RESOLVE_HD static inline int query_last_point(const View &V, const float *Tcw_cur, bool forward, bool backward, const float *pos, int valid,
                                                    int octave, float th, MatchQuery &Q)
{
    const Camera &C = V.C;
    const float min_x = V.min_x, max_x = V.max_x, min_y = V.min_y, max_y = V.max_y;
    if (!valid) return 0;
    if (octave < 0 || octave >= V.nlevels) return -1;
    float xc[3];
    rt_apply(Tcw_cur, pos, xc);
    const float invzc = (float)(1.0 / (double)xc[2]);
    if (invzc < 0) return 0;
    const float u = C.fx * xc[0] * invzc + C.cx;
    const float v = C.fy * xc[1] * invzc + C.cy;
    if (u < min_x || u > max_x) return 0;
    if (v < min_y || v > max_y) return 0;
    const int oct = octave;
    const float radius = th * V.sf[oct];
    Q.u = u; Q.v = v; Q.r = radius; Q.flags = 1 | 2;
    Q.ur = u - C.bf * invzc; Q.ur_rad = radius;
    if (forward) { Q.min_level = oct; Q.max_level = -1; }
    else if (backward) { Q.min_level = 0; Q.max_level = oct; }
    else { Q.min_level = oct - 1; Q.max_level = oct + 1; }
    return 1;
}
// Returns -1 on a bad octave.
static inline int build_queries_last(const View &V, const float *Tcw_cur, const float *Tcw_last, int n_last, const float *last_pos, const uint8_t *last_desc,
                                     const int32_t *last_valid, const int32_t *last_octave, float th, int mono, std::vector<MatchQuery> &q,
                                     std::vector<uint8_t> &qd)
{
    bool forward, backward;
    last_motion(V.C, Tcw_cur, Tcw_last, mono, forward, backward);
    q.assign(n_last > 0 ? n_last : 0, NO_QUERY);
    qd.assign((size_t)32 * (n_last > 0 ? n_last : 1), 0);
    for (int i = 0; i < n_last; i++) {
        const int rc = query_last_point(V, Tcw_cur, forward, backward, last_pos + 3 * i, last_valid[i], last_octave[i], th, q[i]);
        if (rc < 0) return -1;
        if (rc > 0) memcpy(&qd[(size_t)32 * i], last_desc + (size_t)32 * i, 32);
    }
    return 0;
}

// ORBmatcher::SearchByProjection(F, vpMapPoints, th), src/ORBmatcher.cc:49-70: the loop body for one map point.
// Q must hold NO_QUERY; returns -1 on a bad predicted level.
ORBFE_RESOLVE_HD static inline int query_track_point(const float *sf, int nlevels, const orbfe_track_point &pt, float th, MatchQuery &Q)
{
    const bool b_factor = th != 1.0;
    if (!pt.in_view) return 0;
    const int lvl = pt.level;
    if (lvl < 0 || lvl >= nlevels) return -1;
    float r = pt.view_cos > 0.998 ? 2.5f : 4.0f; // RadiusByViewingCos, :129-135
    if (b_factor) r *= th;
    Q.u = pt.proj_x; Q.v = pt.proj_y; Q.r = r * sf[lvl];
    Q.min_level = lvl - 1; Q.max_level = lvl; Q.flags = 1 | 2;
    Q.ur = pt.proj_xr; Q.ur_rad = r * sf[lvl];
    return 1;
}
// Returns -1 on a bad predicted level.
static inline int build_queries_points(const float *sf, int nlevels, int n_pts, const orbfe_track_point *pts, const uint8_t *pt_desc, float th,
                                       std::vector<MatchQuery> &q, std::vector<uint8_t> &qd)
{
    q.assign(n_pts > 0 ? n_pts : 0, NO_QUERY);
    qd.assign((size_t)32 * (n_pts > 0 ? n_pts : 1), 0);
    for (int i = 0; i < n_pts; i++) {
        const int rc = query_track_point(sf, nlevels, pts[i], th, q[i]);
        if (rc < 0) return -1;
        if (rc > 0) memcpy(&qd[(size_t)32 * i], pt_desc + (size_t)32 * i, 32);
    }
    return 0;
}

// ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist), src/ORBmatcher.cc:1484-1527: the loop body for one
// map point of the keyframe (ow = camera_center(Tcw_cur); valid = pMP && !pMP->isBad() && !sAlreadyFound.count(pMP)).
// Q must hold NO_QUERY; returns 1 when the point opens a window.
ORBFE_RESOLVE_HD static inline int query_kf_point(const View &V, const float *Tcw_cur, const float *ow, const float *pos, int valid, float max_distance,
                                                  float min_distance, float th, MatchQuery &Q)
{
    const Camera &C = V.C;
    const int nlevels = V.nlevels;
    const float log_sf = V.log_sf;
    const float min_x = V.min_x, max_x = V.max_x, min_y = V.min_y, max_y = V.max_y;
    if (!valid) return 0;
    float xc[3];
    rt_apply(Tcw_cur, pos, xc);
    const float invzc = (float)(1.0 / (double)xc[2]);
    const float u = C.fx * xc[0] * invzc + C.cx;
    const float v = C.fy * xc[1] * invzc + C.cy;
    if (u < min_x || u > max_x) return 0;
    if (v < min_y || v > max_y) return 0;
    float po[3];
    for (int k = 0; k < 3; k++) po[k] = pos[k] - ow[k];
    const float dist3d = norm3(po);
    if (dist3d < 0.8f * min_distance || dist3d > 1.2f * max_distance) return 0;
    const int lvl = predict_scale(max_distance, dist3d, log_sf, nlevels);
    Q.u = u; Q.v = v; Q.r = th * V.sf[lvl]; Q.min_level = lvl - 1; Q.max_level = lvl + 1; Q.flags = 1;
    return 1;
}
static inline void build_queries_kf(const View &V, const float *Tcw_cur, int n_kf, const float *kf_pos, const uint8_t *kf_desc, const int32_t *kf_valid,
                                    const float *kf_max_distance, const float *kf_min_distance, float th, std::vector<MatchQuery> &q,
                                    std::vector<uint8_t> &qd)
{
    float ow[3];
    camera_center(Tcw_cur, ow);
    q.assign(n_kf > 0 ? n_kf : 0, NO_QUERY);
    qd.assign((size_t)32 * (n_kf > 0 ? n_kf : 1), 0);
    for (int i = 0; i < n_kf; i++)
        if (query_kf_point(V, Tcw_cur, ow, kf_pos + 3 * i, kf_valid[i], kf_max_distance[i], kf_min_distance[i], th, q[i]) > 0)
            memcpy(&qd[(size_t)32 * i], kf_desc + (size_t)32 * i, 32);
}

// Sim3 decomposition of the LoopClosing matchers (src/ORBmatcher.cc:293-298, 981-986); see oracle/orb_oracle_match.c
static inline void sim3_to_rt(const float *Scw, float *T)
{
    const double d = (double)Scw[0] * Scw[0] + (double)Scw[1] * Scw[1] + (double)Scw[2] * Scw[2];
    const float scw = (float)sqrt(d);
    const float alpha = (float)(1.0 / (double)scw);
    for (int i = 0; i < 12; i++) T[i] = Scw[i] * alpha;
}
// KeyFrame::IsInImage (src/KeyFrame.cc:604-607): a keyframe's bounds are ints initialised from the frame's floats
ORBFE_RESOLVE_HD static inline bool kf_is_in_image(const View &V, float u, float v)
{
    const float min_x = V.min_x, max_x = V.max_x, min_y = V.min_y, max_y = V.max_y;
    if (V.keyframe) return u >= (float)(int)min_x && u < (float)(int)max_x && v >= (float)(int)min_y && v < (float)(int)max_y;
    return u >= min_x && u < max_x && v >= min_y && v < max_y;
}
// ORBmatcher::Fuse(pKF, vpMapPoints, th), src/ORBmatcher.cc:821-971, and the Sim3 matchers of LoopClosing (SearchByProjection :285-398
// and Fuse :973-1096, T and ow from the decomposed Scw): the loop body for one map point up to GetFeaturesInArea.  The three loops differ in one statement: the
// Sim3 Fuse takes the reciprocal of the depth in double (`double_recip`); their depth tests, float or double, are the same test.
// Q must hold NO_QUERY; returns 1 when the point opens a window, and then *ur is the projection into the right image (u - bf / z).
ORBFE_RESOLVE_HD static inline int query_fuse_point(const View &V, const float *T, const float *ow, int double_recip, const float *pos, const float *normal,
                                                    int valid, float max_distance, float min_distance, float th, MatchQuery &Q, float *ur)
{
    const Camera &C = V.C;
    const int nlevels = V.nlevels;
    const float log_sf = V.log_sf;
    if (!valid) return 0;
    float pc[3];
    rt_apply(T, pos, pc);
    if (pc[2] < 0.0f) return 0;
    const float invz = double_recip ? (float)(1.0 / (double)pc[2]) : 1 / pc[2];
    const float x = pc[0] * invz, y = pc[1] * invz;
    const float u = C.fx * x + C.cx;
    const float v = C.fy * y + C.cy;
    if (!kf_is_in_image(V, u, v)) return 0;
    float po[3];
    for (int k = 0; k < 3; k++) po[k] = pos[k] - ow[k];
    const float dist3d = norm3(po);
    if (dist3d < 0.8f * min_distance || dist3d > 1.2f * max_distance) return 0;
    const double dot = (double)po[0] * normal[0] + (double)po[1] * normal[1] + (double)po[2] * normal[2];
    if (dot < 0.5 * (double)dist3d) return 0;
    const int lvl = predict_scale(max_distance, dist3d, log_sf, nlevels);
    Q.u = u; Q.v = v; Q.r = th * V.sf[lvl]; Q.min_level = lvl - 1; Q.max_level = lvl; Q.flags = 1;
    *ur = u - C.bf * invz;
    return 1;
}
// One direction of ORBmatcher::SearchBySim3 (src/ORBmatcher.cc:1143-1216 / 1218-1291): the loop body for one map point of keyframe A
// up to GetFeaturesInArea on keyframe B.  Taw moves the point into camera A, sRt = [sR|t] from there into camera B; the view is B's.  valid = pMP && !pMP->isBad() && not already matched.  Q must hold NO_QUERY; returns 1 when the point opens a window.
ORBFE_RESOLVE_HD static inline int query_sim3_point(const View &V, const float *Taw, const float *sRt, const float *pos, int valid, float max_distance,
                                                    float min_distance, float th, MatchQuery &Q)
{
    const Camera &C = V.C;
    const int nlevels = V.nlevels;
    const float log_sf = V.log_sf;
    if (!valid) return 0;
    float pa[3], pb[3];
    rt_apply(Taw, pos, pa);
    rt_apply(sRt, pa, pb);
    if ((double)pb[2] < 0.0) return 0;
    const float invz = (float)(1.0 / (double)pb[2]);
    const float x = pb[0] * invz, y = pb[1] * invz;
    const float u = C.fx * x + C.cx, v = C.fy * y + C.cy;
    if (!kf_is_in_image(V, u, v)) return 0;
    const float dist = norm3(pb);
    if (dist < 0.8f * min_distance || dist > 1.2f * max_distance) return 0;
    const int lvl = predict_scale(max_distance, dist, log_sf, nlevels);
    Q.u = u; Q.v = v; Q.r = th * V.sf[lvl]; Q.min_level = lvl - 1; Q.max_level = lvl; Q.flags = 1;
    return 1;
}
// sR12 = s12 * R12; sR21 = (1.0 / s12) * R12.t(); t21 = -sR21 * t12 (src/ORBmatcher.cc:1116-1119) as two [sR|t] rows of 4
static inline void sim3_pair(float s12, const float *R12, const float *t12, float *A12, float *A21)
{
    const float inv_s = (float)(1.0 / (double)s12);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) { A12[4 * i + j] = R12[3 * i + j] * s12; A21[4 * i + j] = R12[3 * j + i] * inv_s; }
    for (int i = 0; i < 3; i++) {
        A12[4 * i + 3] = t12[i];
        const float t0 = (A21[4 * i] * t12[0] + A21[4 * i + 1] * t12[1]) + A21[4 * i + 2] * t12[2];
        A21[4 * i + 3] = -t0;
    }
}
// The chi-square gates of Fuse on one candidate keypoint (src/ORBmatcher.cc:905-930): reprojection error in stereo where the keypoint
// has a right coordinate (kur >= 0; pass -1 for a keyframe without mvuRight), else monocular; sf_lv = mvScaleFactors[kpLevel]
ORBFE_RESOLVE_HD static inline bool fuse_chi2_passes(float u, float v, float ur, float kx, float ky, float kur, float sf_lv)
{
    const float inv_sigma2 = 1.0f / (sf_lv * sf_lv); // mvInvLevelSigma2 (src/ORBextractor.cc:419-425)
    const float ex = u - kx, ey = v - ky;
    if (kur >= 0) {
        const float er = ur - kur;
        const float e2 = ex * ex + ey * ey + er * er;
        return !((double)(e2 * inv_sigma2) > 7.8);
    }
    const float e2 = ex * ex + ey * ey;
    return !((double)(e2 * inv_sigma2) > 5.99);
}

// ORBmatcher::SearchForInitialization, src/ORBmatcher.cc:414-421
static inline void build_queries_initialization(int n1, const orbfe_keypoint *keys1, const uint8_t *desc1, const float *prev_matched, int window_size,
                                                std::vector<MatchQuery> &q, std::vector<uint8_t> &qd)
{
    q.assign(n1 > 0 ? n1 : 0, NO_QUERY);
    qd.assign((size_t)32 * (n1 > 0 ? n1 : 1), 0);
    for (int i = 0; i < n1; i++) {
        MatchQuery &Q = q[i];
        const int level1 = keys1[i].octave;
        if (level1 > 0) continue;
        Q.u = prev_matched[2 * i]; Q.v = prev_matched[2 * i + 1]; Q.r = (float)window_size;
        Q.min_level = level1; Q.max_level = level1; Q.flags = 1;
        memcpy(&qd[(size_t)32 * i], desc1 + (size_t)32 * i, 32);
    }
}

// Frame::isInFrustum, src/Frame.cc:256-315, for one map point (ow = camera_center(Tcw))
ORBFE_RESOLVE_HD static inline void frustum_point(const View &V, const float *Tcw, const float *ow, const float *pos, const float *normal, float max_distance,
                                                  float min_distance, float viewing_cos_limit, orbfe_track_point &o)
{
    const Camera &C = V.C;
    const int nlevels = V.nlevels;
    const float log_sf = V.log_sf;
    const float min_x = V.min_x, max_x = V.max_x, min_y = V.min_y, max_y = V.max_y;
    o.in_view = 0; o.proj_x = o.proj_y = o.proj_xr = 0.f; o.level = 0; o.view_cos = 0.f;
    float pc[3];
    rt_apply(Tcw, pos, pc);
    if (pc[2] < 0.0f) return;
    const float invz = 1.0f / pc[2];
    const float u = C.fx * pc[0] * invz + C.cx;
    const float v = C.fy * pc[1] * invz + C.cy;
    if (u < min_x || u > max_x) return;
    if (v < min_y || v > max_y) return;
    float po[3];
    for (int k = 0; k < 3; k++) po[k] = pos[k] - ow[k];
    const float dist = norm3(po);
    if (dist < 0.8f * min_distance || dist > 1.2f * max_distance) return;
    const double dot = (double)po[0] * normal[0] + (double)po[1] * normal[1] + (double)po[2] * normal[2];
    const float view_cos = (float)(dot / (double)dist);
    if (view_cos < viewing_cos_limit) return;
    o.in_view = 1;
    o.proj_x = u; o.proj_xr = u - C.bf * invz; o.proj_y = v;
    o.level = predict_scale(max_distance, dist, log_sf, nlevels);
    o.view_cos = view_cos;
}
// ... and for n of them
static inline void is_in_frustum(const View &V, const float *Tcw, int n, const float *pos, const float *normal, const float *max_distance,
                                 const float *min_distance, float viewing_cos_limit, orbfe_track_point *out)
{
    float ow[3];
    camera_center(Tcw, ow);
    for (int i = 0; i < n; i++)
        frustum_point(V, Tcw, ow, pos + 3 * i, normal + 3 * i, max_distance[i], min_distance[i], viewing_cos_limit, out[i]);
}

enum { HISTO_LENGTH = 30, TH_LOW = 50, TH_HIGH = 100, TOPK = 4 };
typedef unsigned long long ckey_t;
static const ckey_t NO_KEY = ~0ull;

ORBFE_RESOLVE_HD static inline int key_dist(ckey_t k) { return (int)(k >> 36); }
ORBFE_RESOLVE_HD static inline int key_idx(ckey_t k) { return (int)((k >> 8) & 0xffffu); }
ORBFE_RESOLVE_HD static inline int key_level(ckey_t k) { return (int)(k & 0xffu); }

// ORBmatcher::ComputeThreeMaxima, src/ORBmatcher.cc:1597-1638, on the bin sizes.  The reference keeps a running top three with
// strict comparisons, i.e. the three largest NON-EMPTY bins in the order (size descending, index ascending); written here as
// three selections of the largest remaining (size, -index) key instead of the reference's shifting if-chain (the oracle and
// oracle/literal_matchers.py keep that form, so the two formulations check each other).
ORBFE_RESOLVE_HD static inline void three_maxima(const int32_t *sizes, int L, int *ind1, int *ind2, int *ind3)
{
    int ind[3] = {-1, -1, -1};
    int32_t val[3] = {0, 0, 0};
    for (int r = 0; r < 3; r++) {
        long long best = -1;
        for (int i = 0; i < L; i++) {
            if (sizes[i] <= 0 || i == ind[0] || i == ind[1]) continue;
            const long long key = ((long long)sizes[i] << 32) | (long long)(0x7fffffff - i);
            if (key > best) { best = key; ind[r] = i; val[r] = sizes[i]; }
        }
        if (best < 0) break;
    }
    if ((float)val[1] < 0.1f * (float)val[0]) { ind[1] = -1; ind[2] = -1; } // :1628-1637
    else if ((float)val[2] < 0.1f * (float)val[0]) ind[2] = -1;
    *ind1 = ind[0]; *ind2 = ind[1]; *ind3 = ind[2];
}

ORBFE_RESOLVE_HD static inline int rot_bin(float a1, float a2) // Q8: 30 slots, bin = round(rot / 30): the reference's three float statements (:1438-1443), the same in any restatement
{
    const float factor = 1.0f / HISTO_LENGTH;
    float rot = a1 - a2;
    if (rot < 0.0) rot += 360.0f;
    int bin = (int)roundf(rot * factor);
    if (bin == HISTO_LENGTH) bin = 0;
    return bin;
}

struct RotHist {
    std::vector<int> v[HISTO_LENGTH];
    void three(int &i1, int &i2, int &i3) const
    {
        int32_t sizes[HISTO_LENGTH];
        for (int i = 0; i < HISTO_LENGTH; i++) sizes[i] = (int32_t)v[i].size();
        three_maxima(sizes, HISTO_LENGTH, &i1, &i2, &i3);
    }
};

// Where the replay gets a query's candidates from.  topk[q * TOPK ..]: ascending, NO_KEY padded; n_static[q]: how many keys
// passed the static filters (> TOPK: the top-K block is a prefix).  full(q, out): every key of the query, unfiltered and
// unsorted (the device's list); called at most for the few queries whose top-K block ran out.
struct CandidateSource {
    const ckey_t *topk = nullptr;
    const int32_t *n_static = nullptr;
    const uint8_t *blocked0 = nullptr; // static filter: keypoints blocked before the call (may be null)
    bool drop_gated = false;           // static filter: keys with dist >= 256 (failed the mvuRight gate)
    void *user = nullptr;
    int (*full)(void *user, int q, std::vector<ckey_t> &out) = nullptr; // returns 0 on success
    int error = 0;
    std::vector<ckey_t> scratch;

    // candidates of query q in ascending order after the static filters; `complete` = nothing beyond them exists
    const ckey_t *begin(int q, int &n, bool &complete)
    {
        const ckey_t *p = topk + (size_t)q * TOPK;
        n = 0;
        while (n < TOPK && p[n] != NO_KEY) n++;
        complete = n_static[q] <= TOPK;
        return p;
    }
    // the full, statically filtered, ascending list (fallback)
    const ckey_t *all(int q, int &n)
    {
        scratch.clear();
        if (!full || full(user, q, scratch) != 0) { error = 1; n = 0; return scratch.data(); }
        size_t w = 0;
        for (size_t i = 0; i < scratch.size(); i++) {
            const ckey_t k = scratch[i];
            if (drop_gated && key_dist(k) >= 256) continue;
            if (blocked0 && blocked0[key_idx(k)]) continue;
            scratch[w++] = k;
        }
        scratch.resize(w);
        std::sort(scratch.begin(), scratch.end());
        n = (int)scratch.size();
        return scratch.data();
    }
};

// first (and second) candidate of query q for which skip(key) is false, in ascending key order
template <class Skip>
static inline void first_two(CandidateSource &src, int q, Skip skip, ckey_t &best, ckey_t &second, bool want_second)
{
    best = second = NO_KEY;
    int n;
    bool complete;
    const ckey_t *c = src.begin(q, n, complete);
    for (int pass = 0; pass < 2; pass++) {
        for (int k = 0; k < n; k++) {
            if (skip(c[k])) continue;
            if (best == NO_KEY) { best = c[k]; if (!want_second) return; }
            else { second = c[k]; return; }
        }
        if (complete || pass == 1) return;
        best = second = NO_KEY; // the prefix ran out before both were found: replay on the full list
        c = src.all(q, n);
    }
}

// ---- ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono), src/ORBmatcher.cc:1324-1466: accept rules ----
// has_obs[k] in/out scratch (initially: keypoint k holds a point with Observations() > 0); cur_angle = mvKeysUn[k].angle
static inline int resolve_last(CandidateSource &src, int n_last, const int32_t *last_obs, const float *last_angle, int n_cur,
                               const float *cur_angle, size_t cur_angle_stride, std::vector<uint8_t> &has_obs, int check_ori, int32_t *cur_match)
{
    for (int k = 0; k < n_cur; k++) cur_match[k] = -1;
    RotHist rh;
    int nm = 0;
    for (int i = 0; i < n_last; i++) {
        ckey_t best, second;
        first_two(src, i, [&](ckey_t k) { return has_obs[key_idx(k)] != 0; }, best, second, false);
        if (best != NO_KEY && key_dist(best) <= TH_HIGH) {
            const int bi = key_idx(best);
            cur_match[bi] = i;
            has_obs[bi] = last_obs[i] > 0;
            nm++;
            if (check_ori) rh.v[rot_bin(last_angle[i], *(const float *)((const char *)cur_angle + cur_angle_stride * bi))].push_back(bi);
        }
    }
    if (check_ori) {
        int i1, i2, i3;
        rh.three(i1, i2, i3);
        for (int b = 0; b < HISTO_LENGTH; b++)
            if (b != i1 && b != i2 && b != i3)
                for (int idx : rh.v[b]) { cur_match[idx] = -1; nm--; }
    }
    return nm;
}

// ---- ORBmatcher::SearchByProjection(F, vpMapPoints, th), src/ORBmatcher.cc:43-127 ----
static inline int resolve_points(CandidateSource &src, int n_pts, const int32_t *pt_obs, int n_cur, std::vector<uint8_t> &has_obs, float nnratio,
                                 int32_t *cur_match)
{
    for (int k = 0; k < n_cur; k++) cur_match[k] = -1;
    int nm = 0;
    for (int i = 0; i < n_pts; i++) {
        ckey_t best, second; // two smallest (dist, order) keys == best / second of the reference's loop
        first_two(src, i, [&](ckey_t k) { return has_obs[key_idx(k)] != 0; }, best, second, true);
        if (best == NO_KEY) continue;
        const int best_dist = key_dist(best), best_level = key_level(best);
        const int best_dist2 = second != NO_KEY ? key_dist(second) : 256, best_level2 = second != NO_KEY ? key_level(second) : -1;
        if (best_dist <= TH_HIGH) {
            if (best_level == best_level2 && (float)best_dist > nnratio * (float)best_dist2) continue;
            cur_match[key_idx(best)] = i;
            has_obs[key_idx(best)] = pt_obs[i] > 0;
            nm++;
        }
    }
    return nm;
}

// ---- ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist), src/ORBmatcher.cc:1468-1595 ----
static inline int resolve_kf(CandidateSource &src, int n_kf, const float *kf_angle, int n_cur, const float *cur_angle, size_t cur_angle_stride,
                             std::vector<uint8_t> &has_pt, int orb_dist, int check_ori, int32_t *cur_match)
{
    for (int k = 0; k < n_cur; k++) cur_match[k] = -1;
    RotHist rh;
    int nm = 0;
    for (int i = 0; i < n_kf; i++) {
        ckey_t best, second;
        first_two(src, i, [&](ckey_t k) { return has_pt[key_idx(k)] != 0; }, best, second, false);
        if (best != NO_KEY && key_dist(best) <= orb_dist) {
            const int bi = key_idx(best);
            cur_match[bi] = i;
            has_pt[bi] = 1;
            nm++;
            if (check_ori) rh.v[rot_bin(kf_angle[i], *(const float *)((const char *)cur_angle + cur_angle_stride * bi))].push_back(bi);
        }
    }
    if (check_ori) {
        int i1, i2, i3;
        rh.three(i1, i2, i3);
        for (int b = 0; b < HISTO_LENGTH; b++)
            if (b != i1 && b != i2 && b != i3)
                for (int idx : rh.v[b]) { cur_match[idx] = -1; nm--; }
    }
    return nm;
}

// ---- ORBmatcher::SearchForInitialization, src/ORBmatcher.cc:400-515 ----
// angle1 / angle2 = mvKeysUn[].angle of the two frames (strided), xy2 = mvKeysUn[].pt of frame 2 (x at xy2, y 4 bytes later)
static inline int resolve_initialization(CandidateSource &src, int n1, int n2, const float *angle1, size_t stride1, const float *angle2, size_t stride2,
                                         const float *xy2, float nnratio, int check_ori, float *prev_matched, int32_t *matches12)
{
    std::vector<int> matched_dist(n2 > 0 ? n2 : 1, INT_MAX), matches21(n2 > 0 ? n2 : 1, -1);
    for (int i = 0; i < n1; i++) matches12[i] = -1;
    RotHist rh;
    int nm = 0;
    for (int i1 = 0; i1 < n1; i1++) {
        ckey_t best, second;
        first_two(src, i1, [&](ckey_t k) { return matched_dist[key_idx(k)] <= key_dist(k); }, best, second, true); // :437-438
        if (best == NO_KEY) continue;
        const int best_dist = key_dist(best), best_dist2 = second != NO_KEY ? key_dist(second) : INT_MAX, bi = key_idx(best);
        if (best_dist <= TH_LOW && (float)best_dist < (float)best_dist2 * nnratio) {
            if (matches21[bi] >= 0) { matches12[matches21[bi]] = -1; nm--; }
            matches12[i1] = bi;
            matches21[bi] = i1;
            matched_dist[bi] = best_dist;
            nm++;
            if (check_ori)
                rh.v[rot_bin(*(const float *)((const char *)angle1 + stride1 * i1), *(const float *)((const char *)angle2 + stride2 * bi))].push_back(i1);
        }
    }
    if (check_ori) {
        int i1, i2, i3;
        rh.three(i1, i2, i3);
        for (int b = 0; b < HISTO_LENGTH; b++) {
            if (b == i1 || b == i2 || b == i3) continue;
            for (int idx1 : rh.v[b])
                if (matches12[idx1] >= 0) { matches12[idx1] = -1; nm--; }
        }
    }
    for (int i1 = 0; i1 < n1; i1++)
        if (matches12[i1] >= 0) {
            const float *p = (const float *)((const char *)xy2 + stride2 * matches12[i1]);
            prev_matched[2 * i1] = p[0];
            prev_matched[2 * i1 + 1] = p[1];
        }
    return nm;
}

} // namespace orbfe_resolve
