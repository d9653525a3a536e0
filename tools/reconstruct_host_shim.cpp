// reconstruct_host_shim.cpp -- ORB_SLAM2::ReconstructInitial of orbslam2_amd/host/Initializer.h behind one C symbol, so that
// tools/bench_matchers.py --reconstruct can run the host form in its own process (g++ -O2 -ffp-contract=off -shared; built into
// $BENCH_OUT by the tool, never shipped).
#include "../orbslam2_amd/host/Initializer.h"

extern "C" int reconstruct_initial_host(const orbfe_keypoint *keys1, int n1, const orbfe_keypoint *keys2, int n2, const int32_t *pairs, int N, const float *H21,
                                        const float *F21, const float *score, const int32_t *best, const uint8_t *inliers_h, const uint8_t *inliers_f, const float *K,
                                        float sigma, int min_triangulated, int model, int32_t *out_model, float *hyp_R, float *hyp_t, int32_t *ngood,
                                        float *cos_parallax, int32_t *result, int32_t *choice, float *R21, float *t21, float *p3d, uint8_t *triangulated, uint8_t *codes)
{
    return ORB_SLAM2::ReconstructInitial(keys1, n1, keys2, n2, pairs, N, H21, F21, score, best, inliers_h, inliers_f, K, sigma, min_triangulated, model, out_model, hyp_R,
                                         hyp_t, ngood, cos_parallax, result, choice, R21, t21, p3d, triangulated, codes);
}
