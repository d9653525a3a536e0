// triangulate_host_shim.cpp -- orbslam2_amd/host/Triangulate.h behind one C symbol, so that tools/bench_matchers.py --create-new-map-points can
// run the host form in its own process (g++ -O2 -ffp-contract=off -shared; built into $BENCH_OUT by the tool, never shipped).
#include "../orbslam2_amd/host/Triangulate.h"

extern "C" int triangulate_pairs_host(const orbfe_newpoint_keyframe *kf1, const orbfe_newpoint_keyframe *kf2, float mbf, float ratio_factor,
                                      const int32_t *pairs, const int32_t *npairs, int max_pairs, const float *scale, const float *sigma2, int nlevels,
                                      uint8_t *code, float *x3d, int32_t *new_points, int32_t *nnew, float *pos, int n_rows, int32_t *rows_used,
                                      int patch_has_mp)
{
    return ORB_SLAM2::TriangulatePairs(kf1, kf2, mbf, ratio_factor, pairs, npairs, max_pairs, scale, sigma2, nlevels, code, x3d, new_points, nnew, pos, n_rows,
                                       rows_used, patch_has_mp);
}
