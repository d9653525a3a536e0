// TEST-ONLY: runs the device building blocks of orbslam2_amd/csrc/orbfe_lba_blocks.hpp one at a time, so that tests/test_lba_blocks.py
// can compare each with a reference (tests/lba_model.py, math.fsum).  Compiled with the product's flags; nothing here is linked into
// liborbfe.so.
//
// lba_blocks_edges: one thread per edge calls lba_edge_blocks on zeroed accumulators: the edge's own Hll (6), b_l (3) and the 48
//                   doubles of its linearisation (Hpl, its share of Hpp and of b_p) -- 57 doubles per edge.
// lba_blocks_reduce: lba_kernel's test-only instances (reduced system in LDS or in HBM) on a whole problem: vertices, edges, the counting
//                   sort, round 1's first linearisation (lba_linearize) and the Schur reduction of lba_solve at lambda's start value;
//                   returns Hll | b_l per point, the reduced system as it goes into the factorisation, lambda and the system's size.
// lba_blocks_ldlt:  one workgroup of LBA_THREADS threads, as lba_kernel calls it, runs lba_ldlt_solve on an (n + 1) x n system in HBM.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "orbfe_lba_blocks.hpp"

namespace {

constexpr int EDGE_IN = 16, EDGE_OUT = 57; // pose (7), X (3), obs (3), stereo, information, robust

__global__ void edges_kernel(int n, const double *__restrict__ in, const double *__restrict__ cam5, double *__restrict__ out)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const double *pi = in + (size_t)e * EDGE_IN;
    Se3 q;
    q.x = pi[0]; q.y = pi[1]; q.z = pi[2]; q.w = pi[3]; q.t[0] = pi[4]; q.t[1] = pi[5]; q.t[2] = pi[6];
    const CamD cam = {cam5[0], cam5[1], cam5[2], cam5[3], cam5[4]};
    const double X[3] = {pi[7], pi[8], pi[9]}, obs[3] = {pi[10], pi[11], pi[12]};
    double H[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0}, lin[LBA_LIN];
    for (int k = 0; k < LBA_LIN; k++) lin[k] = 0.0;
    lba_edge_blocks(q, cam, X, obs, pi[13] != 0.0, pi[14], pi[15] != 0.0, cam5[5], cam5[6], H, b, lin);
    double *po = out + (size_t)e * EDGE_OUT;
    for (int k = 0; k < 6; k++) po[k] = H[k];
    for (int k = 0; k < 3; k++) po[6 + k] = b[k];
    for (int k = 0; k < LBA_LIN; k++) po[9 + k] = lin[k];
}

__global__ __launch_bounds__(LBA_THREADS) void ldlt_kernel(double *S, int n, int *ok)
{
    const bool solved = lba_ldlt_solve<LBA_THREADS>(S, n);
    if (threadIdx.x == 0) *ok = solved ? 1 : 0;
}

} // namespace

extern "C" int lba_blocks_edges(int n, const double *in, const double *cam7 /* fx fy cx cy bf delta_mono delta_stereo */, double *out)
{
    if (n <= 0) return 0;
    double *d_in = nullptr, *d_cam = nullptr, *d_out = nullptr;
    int rc = -1;
    if (hipMalloc(&d_in, sizeof(double) * EDGE_IN * n) == hipSuccess && hipMalloc(&d_cam, sizeof(double) * 7) == hipSuccess &&
        hipMalloc(&d_out, sizeof(double) * EDGE_OUT * n) == hipSuccess &&
        hipMemcpy(d_in, in, sizeof(double) * EDGE_IN * n, hipMemcpyHostToDevice) == hipSuccess &&
        hipMemcpy(d_cam, cam7, sizeof(double) * 7, hipMemcpyHostToDevice) == hipSuccess) {
        hipLaunchKernelGGL(edges_kernel, dim3((n + 63) / 64), dim3(64), 0, nullptr, n, d_in, d_cam, d_out);
        if (hipDeviceSynchronize() == hipSuccess && hipMemcpy(out, d_out, sizeof(double) * EDGE_OUT * n, hipMemcpyDeviceToHost) == hipSuccess) rc = 0;
    }
    (void)hipFree(d_in); (void)hipFree(d_cam); (void)hipFree(d_out);
    return rc;
}

extern "C" int lba_blocks_ldlt(double *S /* (n + 1) x n, in/out */, int n, int *ok)
{
    double *d_S = nullptr;
    int *d_ok = nullptr;
    const size_t bytes = sizeof(double) * ((size_t)(n + 1) * n + 1);
    int rc = -1;
    if (hipMalloc(&d_S, bytes) == hipSuccess && hipMalloc(&d_ok, sizeof(int)) == hipSuccess &&
        hipMemcpy(d_S, S, bytes - sizeof(double), hipMemcpyHostToDevice) == hipSuccess) {
        hipLaunchKernelGGL(ldlt_kernel, dim3(1), dim3(LBA_THREADS), 0, nullptr, d_S, n, d_ok);
        if (hipDeviceSynchronize() == hipSuccess && hipMemcpy(S, d_S, bytes - sizeof(double), hipMemcpyDeviceToHost) == hipSuccess &&
            hipMemcpy(ok, d_ok, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess)
            rc = 0;
    }
    (void)hipFree(d_S); (void)hipFree(d_ok);
    return rc;
}

extern "C" int lba_blocks_reduce(int in_lds, int n_kfs, const int32_t *kf_n, const void *keys /* KeyPointPOD[sum kf_n] */, const float *u_right,
                                 const uint8_t *role, const float *Tcw, int n_pts, const int32_t *obs_off, const int32_t *obs_kf,
                                 const int32_t *obs_idx, int n_obs, const float *pos, const float *cam5, const float *inv_sigma2, int nlevels,
                                 double *p_lin /* [n_pts][9] */, double *system /* [(6 F + 1) * 6 F], F = role-1 keyframes */, double *lambda,
                                 int32_t *n_red, int32_t *status)
{
    size_t n_keys = 0;
    int max_free = 0;
    for (int k = 0; k < n_kfs; k++) { n_keys += (size_t)kf_n[k]; max_free += role[k] == ORBFE_BA_LOCAL; }
    if (in_lds && max_free > ORBFE_LBA_LDS_KEYFRAMES) return -2;
    LbaArgs a = {};
    a.n_kfs = n_kfs; a.max_free = max_free; a.n_pts = n_pts; a.n_rows = n_pts; a.n_obs = n_obs; a.nlevels = nlevels;
    for (int l = 0; l < ORBFE_MAX_LEVELS; l++) a.inv_sigma2[l] = l < nlevels ? inv_sigma2[l] : 0.f;
    a.fx = cam5[0]; a.fy = cam5[1]; a.cx = cam5[2]; a.cy = cam5[3]; a.bf = cam5[4];
    a.delta_mono = (double)(float)std::sqrt(5.991);
    a.delta_stereo = (double)(float)std::sqrt(7.815);
    // inputs and outputs of the call in one block, then the kernel's scratch (with the system in HBM in both variants: the LDS one copies it out)
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t o_rec = 0, o_keys = up(o_rec + sizeof(orbfe_ba_keyframe) * n_kfs), o_ur = up(o_keys + sizeof(KeyPointPOD) * n_keys),
                 o_role = up(o_ur + sizeof(float) * n_keys), o_T = up(o_role + n_kfs), o_off = up(o_T + sizeof(float) * 16 * n_kfs),
                 o_kf = up(o_off + sizeof(int32_t) * (n_pts + 1)), o_idx = up(o_kf + sizeof(int32_t) * n_obs), o_pos = up(o_idx + sizeof(int32_t) * n_obs),
                 o_code = up(o_pos + sizeof(float) * 3 * n_pts), o_erase = up(o_code + n_obs), o_cnt = up(o_erase + sizeof(int32_t) * 2 * n_obs),
                 o_info = up(o_cnt + 2 * sizeof(int32_t)), o_scratch = up(o_info + sizeof(orbfe_lba_info));
    const size_t bytes = o_scratch + lba_carve(a, nullptr, true);
    uint8_t *db = nullptr;
    if (hipMalloc(&db, bytes) != hipSuccess) return -1;
    std::vector<uint8_t> host(o_scratch, 0);
    uint8_t *hb = host.data();
    orbfe_ba_keyframe *rec = (orbfe_ba_keyframe *)(hb + o_rec);
    size_t at = 0;
    for (int k = 0; k < n_kfs; k++) {
        rec[k].keys_un = (const orbfe_keypoint *)(db + o_keys) + at;
        rec[k].u_right = (const float *)(db + o_ur) + at;
        rec[k].n = kf_n[k];
        at += (size_t)kf_n[k];
    }
    memcpy(hb + o_keys, keys, sizeof(KeyPointPOD) * n_keys);
    memcpy(hb + o_ur, u_right, sizeof(float) * n_keys);
    memcpy(hb + o_role, role, n_kfs);
    memcpy(hb + o_T, Tcw, sizeof(float) * 16 * n_kfs);
    memcpy(hb + o_off, obs_off, sizeof(int32_t) * (n_pts + 1));
    memcpy(hb + o_kf, obs_kf, sizeof(int32_t) * n_obs);
    memcpy(hb + o_idx, obs_idx, sizeof(int32_t) * n_obs);
    memcpy(hb + o_pos, pos, sizeof(float) * 3 * n_pts);
    a.kfs = (const orbfe_ba_keyframe *)(db + o_rec); a.role = db + o_role; a.Tcw = (float *)(db + o_T); a.row = nullptr;
    a.obs_off = (const int32_t *)(db + o_off); a.obs_kf = (const int32_t *)(db + o_kf); a.obs_idx = (const int32_t *)(db + o_idx);
    a.pos = (float *)(db + o_pos); a.obs_kfs = nullptr; a.edge_code = db + o_code; a.edge_chi2 = nullptr; a.erase = (int32_t *)(db + o_erase);
    a.n_erase = (int32_t *)(db + o_cnt); a.status = (int32_t *)(db + o_cnt) + 1; a.info = (orbfe_lba_info *)(db + o_info);
    lba_carve(a, db + o_scratch, true);
    int rc = -1;
    orbfe_lba_info info;
    if (hipMemset(db, 0, bytes) == hipSuccess && hipMemcpy(db, hb, o_scratch, hipMemcpyHostToDevice) == hipSuccess) {
        if (in_lds) {
            if (hipFuncSetAttribute((const void *)lba_kernel<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LBA_LDS_REQUEST) != hipSuccess) { (void)hipFree(db); return -3; }
            hipLaunchKernelGGL((lba_kernel<true, true>), dim3(1), dim3(LBA_THREADS), lba_system_bytes(max_free) < 8 ? 8 : lba_system_bytes(max_free), nullptr, a);
        } else {
            hipLaunchKernelGGL((lba_kernel<false, true>), dim3(1), dim3(LBA_THREADS), 8, nullptr, a);
        }
        if (hipDeviceSynchronize() == hipSuccess && hipMemcpy(&info, a.info, sizeof(info), hipMemcpyDeviceToHost) == hipSuccess &&
            hipMemcpy(status, a.status, sizeof(int32_t), hipMemcpyDeviceToHost) == hipSuccess &&
            hipMemcpy(p_lin, a.p_lin, sizeof(double) * LBA_PT * n_pts, hipMemcpyDeviceToHost) == hipSuccess &&
            hipMemcpy(system, a.system, lba_system_bytes(info.n_free), hipMemcpyDeviceToHost) == hipSuccess) {
            *lambda = info.lambda_last;
            *n_red = info.n_free;
            rc = 0;
        }
    }
    (void)hipFree(db);
    return rc;
}
