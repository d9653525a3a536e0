// map_point_host_shim.cpp -- orbslam2_amd/host/MapPointUpdate.h behind one C symbol, so that tools/bench_matchers.py --map-points can time the
// host form in its own process (g++ -O2 -ffp-contract=off -shared; built into $BENCH_OUT by the tool, never shipped).
#include "../orbslam2_amd/host/MapPointUpdate.h"

extern "C" int map_point_update_host(const orbfe_obs_keyframe *kfs, int n_kfs, int n_upd, const int32_t *row, int n_rows, const int32_t *obs_off,
                                     const int32_t *obs_kf, const int32_t *obs_idx, int n_obs, const int32_t *ref, int what, const float *scale, int nlevels,
                                     const float *pos, float *normal, float *max_distance, float *min_distance, uint8_t *pt_desc, int32_t *best)
{
    return ORB_SLAM2::UpdateMapPoints(kfs, n_kfs, n_upd, row, n_rows, obs_off, obs_kf, obs_idx, n_obs, ref, what, scale, nlevels, pos, normal, max_distance,
                                      min_distance, pt_desc, best);
}
