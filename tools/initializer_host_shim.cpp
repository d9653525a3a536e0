// initializer_host_shim.cpp -- orbslam2_amd/host/Initializer.h behind one C symbol, so that tools/bench_matchers.py --initializer can run the
// host form in its own process (g++ -O2 -ffp-contract=off -shared -pthread; built into $BENCH_OUT by the tool, never shipped).
// threads == 2 is the reference's own split (src/Initializer.cc:103-108): FindHomography and FindFundamental on a std::thread each.
#include <thread>

#include "../orbslam2_amd/host/Initializer.h"

extern "C" int find_homography_fundamental_host(const orbfe_keypoint *keys1, int n1, const orbfe_keypoint *keys2, int n2, const int32_t *pairs, int N,
                                                const int32_t *sets, int iterations, const float *norm1, const float *norm2, float sigma, float *H21, float *F21,
                                                float *score, int32_t *best, uint8_t *inliers_h, uint8_t *inliers_f, int32_t *ninliers, float *all_scores,
                                                int threads)
{
    auto run = [&](int models) {
        return ORB_SLAM2::FindHomographyFundamental(keys1, n1, keys2, n2, pairs, N, sets, iterations, norm1, norm2, sigma, H21, F21, score, best, inliers_h,
                                                    inliers_f, ninliers, all_scores, models);
    };
    if (threads < 2) return run(3);
    int rh = 0, rf = 0;
    std::thread threadH([&] { rh = run(1); }), threadF([&] { rf = run(2); });
    threadH.join();
    threadF.join();
    return rh ? rh : rf;
}
