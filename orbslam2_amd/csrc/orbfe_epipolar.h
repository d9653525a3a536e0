// orbfe_epipolar.h -- the two pieces of two-view geometry that ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:652-819)
// evaluates per call and per candidate, as one text for the synchronous path (orbfe_bow.hip, host) and the device-resident one
// (orbfe_bow_device.hip, the entry point and the kernel): the same role query_kf_point plays in orbfe_match_resolve.h.  Float
// arithmetic in the reference's order; the library is built without FMA contraction and with IEEE division on both sides.
#pragma once

#ifdef __HIPCC__
#define ORBFE_EPI_HD __attribute__((host, device))
#else
#define ORBFE_EPI_HD
#endif

namespace orbfe_epipolar
{

// Epipole in the second image (:658-664): C2 = R2w * Cw1 + t2w as cv::Mat evaluates a small product in float, then the pinhole
// projection.  T2w = [R|t], 3x4 row major.
ORBFE_EPI_HD static inline void epipole(const float *Cw1, const float *T2w, float fx2, float fy2, float cx2, float cy2, float *ex, float *ey)
{
    float C2[3];
    for (int i = 0; i < 3; i++) {
        const float t = (T2w[4 * i] * Cw1[0] + T2w[4 * i + 1] * Cw1[1]) + T2w[4 * i + 2] * Cw1[2];
        C2[i] = t + T2w[4 * i + 3];
    }
    const float invz = 1.0f / C2[2];
    *ex = fx2 * C2[0] * invz + cx2;
    *ey = fy2 * C2[1] * invz + cy2;
}

// The exclusion disc around the epipole for a monocular pair (:740-746): true = too close, the candidate is skipped.
ORBFE_EPI_HD static inline bool inside_epipole_disc(float ex, float ey, float x2, float y2, float scale_kp2)
{
    const float distex = ex - x2, distey = ey - y2;
    return distex * distex + distey * distey < 100 * scale_kp2;
}

// ORBmatcher::CheckDistEpipolarLine (:138-155): float arithmetic left to right, the last comparison in double (3.84 is a double
// literal), a degenerate line rejects.  F12 3x3 row major.
ORBFE_EPI_HD static inline bool check_dist_epipolar_line(float x1, float y1, float x2, float y2, const float *F12, float sigma2_kp2)
{
    const float a = x1 * F12[0] + y1 * F12[3] + F12[6];
    const float b = x1 * F12[1] + y1 * F12[4] + F12[7];
    const float c = x1 * F12[2] + y1 * F12[5] + F12[8];
    const float num = a * x2 + b * y2 + c;
    const float den = a * a + b * b;
    if (den == 0) return false;
    const float dsqr = num * num / den;
    return (double)dsqr < 3.84 * (double)sigma2_kp2;
}

} // namespace orbfe_epipolar
