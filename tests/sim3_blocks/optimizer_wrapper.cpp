// TEST-ONLY: ORB_SLAM2::Optimizer::OptimizeSim3 of orbslam2_amd/host/Optimizer.h behind one C function, so that
// tests/test_sim3_opt_device.py can call the header's wrapper (std::vector in, exception on error) from Python.
#include <cstdint>
#include <exception>
#include <vector>

#include "../../orbslam2_amd/host/Optimizer.h"

// 0 and *n_in on success; -100 when the wrapper threw
extern "C" int sim3_wrapper_optimize(orbfe_context *ctx, const orbfe_keypoint *keys1, int n1, const float *T1w, const float *pos1, const int32_t *valid1,
                                     const orbfe_keypoint *keys2, int n2, const float *T2w, const float *pos2, const int32_t *valid2, float s12,
                                     const float *R12, const float *t12, int32_t *match12, const int32_t *prior12, double *S12, float th2, int fix_scale, int *n_in)
{
    try {
        std::vector<orbfe_keypoint> k1(keys1, keys1 + n1), k2(keys2, keys2 + n2);
        std::vector<float> p1(pos1, pos1 + 3 * (size_t)n1), p2(pos2, pos2 + 3 * (size_t)n2);
        std::vector<int32_t> v1(valid1, valid1 + n1), v2(valid2, valid2 + n2), m(match12, match12 + n1), pr;
        if (prior12) pr.assign(prior12, prior12 + n1);
        *n_in = ORB_SLAM2::Optimizer::OptimizeSim3(ctx, k1, T1w, p1, v1, k2, T2w, p2, v2, s12, R12, t12, m, S12, th2, fix_scale != 0, pr);
        for (int i = 0; i < n1; i++) match12[i] = m[i];
        return 0;
    } catch (const std::exception &) {
        return -100;
    }
}
