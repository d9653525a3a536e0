// TEST-ONLY: runs the device building blocks of orbslam2_amd/csrc/orbfe_pose_blocks.hpp one at a time, so that
// tests/test_pose_blocks.py can compare each with a float64 reference.  Compiled with the product's flags; nothing here is
// linked into liborbfe.so.
//
// Ops 1-4: one wave of 64 lanes per case, every lane computes the same thing (ldlt_step branches on a readfirstlane, so all
// lanes must hold the same matrix), lane 0 writes.  Op 5: one 256-thread workgroup per case runs eval_pass<256, true> and
// eval_pass<256, false> over the same edge table.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <vector>

#include "orbfe_pose_blocks.hpp"

namespace {

enum { OP_FROM_CV = 1, OP_EXP = 2, OP_MUL = 3, OP_LDLT = 4, OP_EVAL = 5 };
constexpr int IN_STRIDE[5] = {16, 6, 14, 28, 16}, OUT_STRIDE[5] = {23, 7, 7, 7, 62};
constexpr int EV_THREADS = 256, EV_MAX_SLOTS = 1024, EV_LEVELS = 8;

__device__ inline Se3 load_se3(const double *p) { Se3 q; q.x = p[0]; q.y = p[1]; q.z = p[2]; q.w = p[3]; q.t[0] = p[4]; q.t[1] = p[5]; q.t[2] = p[6]; return q; }
__device__ inline void store_se3(const Se3 &q, double *p) { p[0] = q.x; p[1] = q.y; p[2] = q.z; p[3] = q.w; p[4] = q.t[0]; p[5] = q.t[1]; p[6] = q.t[2]; }

__global__ __launch_bounds__(64) void wave_ops_kernel(int op, int n_cases, const double *__restrict__ in, double *__restrict__ out)
{
    const int c = blockIdx.x;
    if (c >= n_cases) return;
    const double *pi = in + (size_t)c * IN_STRIDE[op - 1];
    double *po = out + (size_t)c * OUT_STRIDE[op - 1];
    const bool w = threadIdx.x == 0;
    if (op == OP_FROM_CV) {
        float T[16], To[16];
#pragma unroll
        for (int k = 0; k < 16; k++) T[k] = (float)pi[k];
        const Se3 q = se3_from_cv(T);
        se3_to_cv(q, To);
        if (w) {
            store_se3(q, po);
            for (int k = 0; k < 16; k++) po[7 + k] = (double)To[k];
        }
    } else if (op == OP_EXP) {
        double u[6];
#pragma unroll
        for (int k = 0; k < 6; k++) u[k] = pi[k];
        const Se3 q = se3_exp(u);
        if (w) store_se3(q, po);
    } else if (op == OP_MUL) {
        const Se3 q = se3_mul(load_se3(pi), load_se3(pi + 7));
        if (w) store_se3(q, po);
    } else if (op == OP_LDLT) {
        double x[6] = {7.0, 7.0, 7.0, 7.0, 7.0, 7.0}; // left as it is when the factor is not positive
        const bool positive = solve_ldlt6(pi, pi[27], x);
        if (w) {
            for (int k = 0; k < 6; k++) po[k] = x[k];
            po[6] = positive ? 1.0 : 0.0;
        }
    }
}

// header of one eval case: n, robust, pose (x y z w t), camera (fx fy cx cy bf), first slot
__global__ __launch_bounds__(EV_THREADS) void eval_kernel(const double *__restrict__ hdr, const KeyPointPOD *__restrict__ keys, const float *__restrict__ u_right,
                                                          const uint8_t *__restrict__ has_point, const float *__restrict__ Xw, uint8_t *__restrict__ outlier,
                                                          const float *__restrict__ inv_sigma2, int cap_max, double *__restrict__ out)
{
    extern __shared__ double s_dyn[];
    double *s_rows = s_dyn;                       // [EV_THREADS/16][32]
    double *s_tot = s_rows + (EV_THREADS / 16) * 32; // [32]
    const double *h = hdr + (size_t)blockIdx.x * 16;
    const int o0 = (int)h[15];
    EdgeTable E;
    E.n = (int)h[0];
    E.cap = (E.n > 0 ? E.n + 3 : 4) & ~3; // as orbfe_enqueue_pose_optimization rounds max_keypoints
    E.keys = keys + o0; E.u_right = u_right + o0; E.has_point = has_point + o0; E.Xw = Xw + (size_t)3 * o0; E.outlier = outlier + o0;
    E.inv_sigma2 = inv_sigma2;
    E.l_f = (float *)(s_tot + 32);
    E.l_st = (uint8_t *)(E.l_f + 7 * (size_t)cap_max);
    const bool robust = h[1] != 0.0;
    const Se3 q = load_se3(h + 2);
    const CamD cam = {h[9], h[10], h[11], h[12], h[13]};
    const double delta_mono = (double)(float)sqrt(5.991), delta_stereo = (double)(float)sqrt(7.815);
    for (int i = threadIdx.x; i < E.n; i += EV_THREADS) { // the staging of pose_opt_kernel, with the caller's outlier marks kept
        const bool has = E.has_point[i] != 0;
        const KeyPointPOD kp = E.keys[i];
        E.l_f[0 * E.cap + i] = E.Xw[3 * (size_t)i];
        E.l_f[1 * E.cap + i] = E.Xw[3 * (size_t)i + 1];
        E.l_f[2 * E.cap + i] = E.Xw[3 * (size_t)i + 2];
        E.l_f[3 * E.cap + i] = kp.x;
        E.l_f[4 * E.cap + i] = kp.y;
        E.l_f[5 * E.cap + i] = E.u_right[i];
        E.l_f[6 * E.cap + i] = has ? inv_sigma2[kp.octave] : 0.f;
        E.l_st[i] = has ? (E.outlier[i] ? 2 : 1) : 0;
    }
    double *po = out + (size_t)blockIdx.x * 62;
    double chi, cnt;
    eval_pass<EV_THREADS, true>(E, q, cam, robust, delta_mono, delta_stereo, s_rows, s_tot, chi, cnt);
    if (threadIdx.x < 29) po[threadIdx.x] = s_tot[threadIdx.x];
    if (threadIdx.x == 0) { po[58] = chi; po[59] = cnt; }
    __syncthreads();
    eval_pass<EV_THREADS, false>(E, q, cam, robust, delta_mono, delta_stereo, s_rows, s_tot, chi, cnt);
    if (threadIdx.x < 29) po[29 + threadIdx.x] = s_tot[threadIdx.x];
    if (threadIdx.x == 0) { po[60] = chi; po[61] = cnt; }
}

struct Dev {
    void *p = nullptr;
    ~Dev() { if (p) (void)hipFree(p); }
    bool up(const void *src, size_t bytes)
    {
        if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) return false;
        return !bytes || !src || hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) == hipSuccess;
    }
};

} // namespace

// what `in` points to for OP_EVAL (host arrays; `total` slots over all cases, inv_sigma2 has 8 levels)
struct pose_blocks_eval_in {
    const double *hdr;
    const KeyPointPOD *keys;
    const float *u_right;
    const uint8_t *has_point;
    const float *Xw;
    const uint8_t *outlier;
    const float *inv_sigma2;
    int32_t total;
};

// Host arrays in, host arrays out; 0 on success, -1 bad argument, -2 HIP error.
extern "C" int pose_blocks_run(int op, int n_cases, const void *in, void *out)
{
    if (op < OP_FROM_CV || op > OP_EVAL || n_cases <= 0 || n_cases > 65535 || !in || !out) return -1;
    const size_t out_bytes = sizeof(double) * OUT_STRIDE[op - 1] * (size_t)n_cases;
    Dev d_out;
    if (!d_out.up(nullptr, out_bytes) || hipMemset(d_out.p, 0, out_bytes) != hipSuccess) return -2;
    if (op != OP_EVAL) {
        Dev d_in;
        if (!d_in.up(in, sizeof(double) * IN_STRIDE[op - 1] * (size_t)n_cases)) return -2;
        hipLaunchKernelGGL(wave_ops_kernel, dim3(n_cases), dim3(64), 0, 0, op, n_cases, (const double *)d_in.p, (double *)d_out.p);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -2;
    } else {
        const pose_blocks_eval_in *e = (const pose_blocks_eval_in *)in;
        if (!e->hdr || !e->keys || !e->u_right || !e->has_point || !e->Xw || !e->outlier || !e->inv_sigma2 || e->total <= 0) return -1;
        int cap_max = 4;
        for (int c = 0; c < n_cases; c++) { // every address the kernel forms is checked here
            const double *h = e->hdr + (size_t)c * 16;
            const int n = (int)h[0], o0 = (int)h[15];
            if (n < 1 || n > EV_MAX_SLOTS || o0 < 0 || (double)n != h[0] || (double)o0 != h[15] || (long long)o0 + n > e->total) return -1;
            for (int i = o0; i < o0 + n; i++)
                if (e->keys[i].octave < 0 || e->keys[i].octave >= EV_LEVELS) return -1;
            cap_max = std::max(cap_max, (n + 3) & ~3);
        }
        const size_t t = (size_t)e->total;
        Dev d_hdr, d_keys, d_ur, d_has, d_xw, d_outl, d_sig;
        if (!d_hdr.up(e->hdr, sizeof(double) * 16 * n_cases) || !d_keys.up(e->keys, sizeof(KeyPointPOD) * t) || !d_ur.up(e->u_right, sizeof(float) * t) ||
            !d_has.up(e->has_point, t) || !d_xw.up(e->Xw, sizeof(float) * 3 * t) || !d_outl.up(e->outlier, t) || !d_sig.up(e->inv_sigma2, sizeof(float) * EV_LEVELS))
            return -2;
        const size_t lds = sizeof(double) * ((EV_THREADS / 16) * 32 + 32) + (size_t)cap_max * (7 * sizeof(float) + 1) + 16; // 34 KiB at most
        hipLaunchKernelGGL(eval_kernel, dim3(n_cases), dim3(EV_THREADS), lds, 0, (const double *)d_hdr.p, (const KeyPointPOD *)d_keys.p, (const float *)d_ur.p,
                           (const uint8_t *)d_has.p, (const float *)d_xw.p, (uint8_t *)d_outl.p, (const float *)d_sig.p, cap_max, (double *)d_out.p);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -2;
    }
    return hipMemcpy(out, d_out.p, out_bytes, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -2;
}
