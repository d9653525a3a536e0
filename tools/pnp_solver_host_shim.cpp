// pnp_solver_host_shim.cpp -- tools/bench_matchers.py --pnp: ORB_SLAM2::PnPRansacHost (orbslam2_amd/host/PnPsolver.h) behind one C symbol,
// for K candidates against one frame, so that the host form can be timed on the CPU.  Returns the sum of the candidates' event counts.
#include "../orbslam2_amd/host/PnPsolver.h"

extern "C" int pnp_ransac_host(const orbfe_keypoint *keys, int n_keys, int K, const int32_t *f_match /* [K][n_keys] */, const float *pos /* [K][n_kf][3] */,
                               const int32_t *valid /* [K][n_kf] */, int n_kf, const uint32_t *draws /* [K][max_its][4] */, int min_inliers, int max_its,
                               int n_iterations, float epsilon, float th2, const int32_t *its_for_n, const float *sigma2, int nlevels, const float *cam)
{
    int events = 0;
    for (int c = 0; c < K; c++) {
        const ORB_SLAM2::PnPRows rows = ORB_SLAM2::PnPRansacHost(keys, n_keys, f_match + (size_t)c * n_keys, pos + (size_t)c * 3 * n_kf, valid + (size_t)c * n_kf, n_kf,
                                                                 draws + (size_t)c * 4 * max_its, n_keys, min_inliers, max_its, n_iterations, epsilon, th2, its_for_n,
                                                                 sigma2, nlevels, cam);
        events += rows.n_events;
    }
    return events;
}
