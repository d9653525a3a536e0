// TEST-ONLY: runs the device building blocks of orbslam2_amd/csrc/orbfe_sim3_blocks.hpp (and solve_ldlt<7> of orbfe_pose_blocks.hpp) one
// at a time, so that tests/test_sim3_blocks.py can compare each with the float64 model (tests/sim3_opt_model.py).  Compiled with the
// product's flags; nothing here is linked into liborbfe.so.
//
// Ops 1-6: one wave of 64 lanes per case, every lane computes the same thing (ldlt_step branches on a readfirstlane, so all lanes must
// hold the same matrix), lane 0 writes.  Op 7: one 256-thread workgroup per case stages its correspondence table in LDS, as
// sim3_opt_kernel holds it, and runs sim3_eval_pass<256> at the given estimate.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "orbfe_sim3_blocks.hpp"

namespace {

enum { OP_FROM_RTS = 1, OP_EXP = 2, OP_MUL = 3, OP_INVERSE = 4, OP_MAP = 5, OP_LDLT7 = 6, OP_EVAL = 7 };
constexpr int IN_STRIDE[7] = {13, 7, 16, 8, 11, 36, 16}, OUT_STRIDE[7] = {8, 8, 8, 8, 3, 8, 39};
constexpr int EV_THREADS = 256, EV_MAX_ROWS = 1024;

__global__ __launch_bounds__(64) void wave_ops_kernel(int op, int n_cases, const double *__restrict__ in, double *__restrict__ out)
{
    const int c = blockIdx.x;
    if (c >= n_cases) return;
    const double *pi = in + (size_t)c * IN_STRIDE[op - 1];
    double *po = out + (size_t)c * OUT_STRIDE[op - 1];
    const bool w = threadIdx.x == 0;
    if (op == OP_FROM_RTS) {
        double R[3][3], t[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int j = 0; j < 3; j++) R[i][j] = pi[3 * i + j];
            t[i] = pi[9 + i];
        }
        const Sim3D S = sim3_from_rts(R, t, pi[12]);
        if (w) sim3_store(S, po);
    } else if (op == OP_EXP) {
        double u[7];
#pragma unroll
        for (int k = 0; k < 7; k++) u[k] = pi[k];
        const Sim3D S = sim3_exp(u);
        if (w) sim3_store(S, po);
    } else if (op == OP_MUL) {
        const Sim3D S = sim3_mul(sim3_load(pi), sim3_load(pi + 8));
        if (w) sim3_store(S, po);
    } else if (op == OP_INVERSE) {
        const Sim3D S = sim3_inverse(sim3_load(pi));
        if (w) sim3_store(S, po);
    } else if (op == OP_MAP) {
        double o[3];
        const double p[3] = {pi[8], pi[9], pi[10]};
        sim3_map(sim3_load(pi), p, o);
        if (w) { po[0] = o[0]; po[1] = o[1]; po[2] = o[2]; }
    } else if (op == OP_LDLT7) {
        double x[7] = {7.0, 7.0, 7.0, 7.0, 7.0, 7.0, 7.0}; // left as it is when the factor is not positive
        const bool positive = solve_ldlt<7>(pi, pi[35], x);
        if (w) {
            for (int k = 0; k < 7; k++) po[k] = x[k];
            po[7] = positive ? 1.0 : 0.0;
        }
    }
}

// header of one eval case: n, fix_scale, estimate (x y z w t s), camera (fx fy cx cy), delta, first row
__global__ __launch_bounds__(EV_THREADS) void eval_kernel(const double *__restrict__ hdr, const float *__restrict__ rows /*[total][12]*/,
                                                          const uint8_t *__restrict__ active, int cap, double *__restrict__ out)
{
    extern __shared__ double s_dyn[];
    double *s_rows = s_dyn;                                // [EV_THREADS/16][40]
    double *s_tot = s_rows + (EV_THREADS / 16) * S3_NVAL;  // [40]
    double *s_sims = s_tot + S3_NVAL;                      // [15][16]
    const double *h = hdr + (size_t)blockIdx.x * 16;
    const int n = (int)h[0], o0 = (int)h[15];
    CorrTable T;
    T.cap = cap;
    T.n = n;
    T.f = (float *)(s_sims + S3_NSIM * S3_SIM_STRIDE);
    T.tag = (uint32_t *)(T.f + 12 * (size_t)cap);
    for (int k = threadIdx.x; k < n; k += EV_THREADS) { // k < n <= cap
        float v[12];
#pragma unroll
        for (int j = 0; j < 12; j++) v[j] = rows[(size_t)(o0 + k) * 12 + j];
        corr_store(T, k, v, k);
        if (!active[o0 + k]) corr_remove(T, k);
    }
    __syncthreads();
    const Sim3D est = sim3_load(h + 2);
    const CamK cam = {h[10], h[11], h[12], h[13]};
    double chi, cnt;
    sim3_eval_pass<EV_THREADS>(T, est, h[1] != 0.0, cam, h[14], s_sims, s_rows, s_tot, chi, cnt);
    double *po = out + (size_t)blockIdx.x * 39;
    if (threadIdx.x < 37) po[threadIdx.x] = s_tot[threadIdx.x];
    if (threadIdx.x == 0) { po[37] = chi; po[38] = cnt; }
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

// what `in` points to for OP_EVAL (host arrays; `total` table rows over all cases)
struct sim3_blocks_eval_in {
    const double *hdr;
    const float *rows;
    const uint8_t *active;
    int32_t total;
};

// Host arrays in, host arrays out; 0 on success, -1 bad argument, -2 HIP error.
extern "C" int sim3_blocks_run(int op, int n_cases, const void *in, void *out)
{
    if (op < OP_FROM_RTS || op > OP_EVAL || n_cases <= 0 || n_cases > 65535 || !in || !out) return -1;
    const size_t out_bytes = sizeof(double) * OUT_STRIDE[op - 1] * (size_t)n_cases;
    Dev d_out;
    if (!d_out.up(nullptr, out_bytes) || hipMemset(d_out.p, 0, out_bytes) != hipSuccess) return -2;
    if (op != OP_EVAL) {
        Dev d_in;
        if (!d_in.up(in, sizeof(double) * IN_STRIDE[op - 1] * (size_t)n_cases)) return -2;
        hipLaunchKernelGGL(wave_ops_kernel, dim3(n_cases), dim3(64), 0, 0, op, n_cases, (const double *)d_in.p, (double *)d_out.p);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -2;
    } else {
        const sim3_blocks_eval_in *e = (const sim3_blocks_eval_in *)in;
        if (!e->hdr || !e->rows || !e->active || e->total <= 0) return -1;
        int cap = 4;
        for (int c = 0; c < n_cases; c++) { // every address the kernel forms is checked here
            const double *h = e->hdr + (size_t)c * 16;
            const int n = (int)h[0], o0 = (int)h[15];
            if (n < 1 || n > EV_MAX_ROWS || o0 < 0 || (double)n != h[0] || (double)o0 != h[15] || (long long)o0 + n > e->total) return -1;
            cap = std::max(cap, (n + 3) & ~3);
        }
        const size_t t = (size_t)e->total;
        Dev d_hdr, d_rows, d_act;
        if (!d_hdr.up(e->hdr, sizeof(double) * 16 * n_cases) || !d_rows.up(e->rows, sizeof(float) * 12 * t) || !d_act.up(e->active, t)) return -2;
        const size_t lds = sizeof(double) * ((EV_THREADS / 16) * S3_NVAL + S3_NVAL + S3_NSIM * S3_SIM_STRIDE) + corr_table_bytes(cap); // 60 KiB at most
        hipLaunchKernelGGL(eval_kernel, dim3(n_cases), dim3(EV_THREADS), lds, 0, (const double *)d_hdr.p, (const float *)d_rows.p, (const uint8_t *)d_act.p, cap,
                           (double *)d_out.p);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -2;
    }
    return hipMemcpy(out, d_out.p, out_bytes, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -2;
}
