// TEST-ONLY: ORB_SLAM2::Optimizer::LocalBundleAdjustment of orbslam2_amd/host/Optimizer.h behind one C function, so that
// tests/test_lba_device.py can call the header's wrapper (std::vector in, exception on error) from Python.
#include <cstdint>
#include <exception>
#include <vector>

#include "../../orbslam2_amd/host/Optimizer.h"

// 0 on success; -100 when the wrapper threw.  keys / u_right: the keyframes' arrays one behind the other, kf_n entries each.
extern "C" int lba_wrapper_adjust(orbfe_context *ctx, int n_kfs, const int32_t *kf_n, const orbfe_keypoint *keys, const float *u_right, const uint8_t *role,
                                  float *Tcw, float *Ow, int n_pts, float *pos, const int32_t *obs_off, const int32_t *obs_kf, const int32_t *obs_idx, int n_obs,
                                  uint8_t *edge_code, double *edge_chi2, int32_t *erase, int32_t *n_erase, orbfe_lba_info *info)
{
    try {
        std::vector<std::vector<orbfe_keypoint>> k(n_kfs);
        std::vector<std::vector<float>> u(n_kfs);
        std::vector<ORB_SLAM2::Optimizer::BAKeyFrame> kfs(n_kfs);
        size_t at = 0;
        for (int i = 0; i < n_kfs; i++) {
            k[i].assign(keys + at, keys + at + kf_n[i]);
            u[i].assign(u_right + at, u_right + at + kf_n[i]);
            kfs[i].vKeysUn = &k[i]; kfs[i].vuRight = &u[i]; kfs[i].role = role[i];
            at += (size_t)kf_n[i];
        }
        std::vector<float> vT(Tcw, Tcw + 16 * (size_t)n_kfs), vOw(Ow, Ow + 3 * (size_t)n_kfs), vP(pos, pos + 3 * (size_t)n_pts);
        const std::vector<int32_t> off(obs_off, obs_off + n_pts + 1), okf(obs_kf, obs_kf + n_obs), oidx(obs_idx, obs_idx + n_obs);
        const ORB_SLAM2::Optimizer::BAResult r = ORB_SLAM2::Optimizer::LocalBundleAdjustment(ctx, kfs, vT, vOw, vP, off, okf, oidx);
        for (size_t i = 0; i < vT.size(); i++) Tcw[i] = vT[i];
        for (size_t i = 0; i < vOw.size(); i++) Ow[i] = vOw[i];
        for (size_t i = 0; i < vP.size(); i++) pos[i] = vP[i];
        for (int j = 0; j < n_obs; j++) { edge_code[j] = r.vEdgeCode[j]; edge_chi2[j] = r.vEdgeChi2[j]; }
        *n_erase = (int32_t)r.vToErase.size();
        for (size_t i = 0; i < r.vToErase.size(); i++) { erase[2 * i] = r.vToErase[i].first; erase[2 * i + 1] = r.vToErase[i].second; }
        *info = r.info;
        return 0;
    } catch (const std::exception &) {
        return -100;
    }
}
