// TEST-ONLY: runs the device building blocks of orbslam2_amd/csrc/orbfe_essential_blocks.hpp one at a time, so that
// tests/test_essential_blocks.py can compare each with the float64 model (tests/essential_graph_model.py).  Compiled with the product's
// flags; nothing here is linked into liborbfe.so.  Every function takes HOST arrays and returns 0, or -1 when a HIP call failed.
//
// eb_log:       one lane per Sim3 (8 doubles each) calls eg_log: 7 doubles each.
// eb_edge:      one workgroup builds the two vertices' perturbation tables (eg_perturb_one, 15 lanes each) and one lane linearises the
//               edge (eg_edge_linearize): e, Ji, Jj = 105 doubles.
// eb_assemble:  one workgroup of EG_THREADS lanes assembles the slots of H and b from per-edge blocks along a plan, as eg_linearize does.
// eb_solve:     one workgroup runs eg_solve on given slots: the workspace in the LDS (in_lds != 0) or in HBM; x in elimination order.
// eb_finish:    eg_recover_pose and eg_correct_point, one lane each.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/orbfe.h"
#include "orbfe_essential_blocks.hpp"

#pragma clang fp contract(off)

namespace {

struct Dev { // device copies freed on scope exit
    std::vector<void *> p;
    bool ok = true;
    template <class T> T *up(const T *h, size_t n)
    {
        void *d = nullptr;
        if (hipMalloc(&d, sizeof(T) * (n ? n : 1)) != hipSuccess) { ok = false; return nullptr; }
        p.push_back(d);
        if (h && n && hipMemcpy(d, h, sizeof(T) * n, hipMemcpyHostToDevice) != hipSuccess) ok = false;
        if (!h && hipMemset(d, 0, sizeof(T) * (n ? n : 1)) != hipSuccess) ok = false;
        return (T *)d;
    }
    template <class T> void down(T *h, const T *d, size_t n)
    {
        if (ok && n && (hipDeviceSynchronize() != hipSuccess || hipMemcpy(h, d, sizeof(T) * n, hipMemcpyDeviceToHost) != hipSuccess)) ok = false;
    }
    ~Dev() { for (void *q : p) (void)hipFree(q); }
};

__global__ void log_kernel(int n, const double *in, double *out)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    double r[7];
    eg_log(sim3_load(in + 8 * (size_t)k), r);
    for (int j = 0; j < 7; j++) out[7 * (size_t)k + j] = r[j];
}

__global__ __launch_bounds__(64) void edge_kernel(const double *C, const double *Si, const double *Sj, int free_i, int free_j, int fix_scale, double *out)
{
    __shared__ double s_pert[2][EG_PERT_STRIDE];
    const int t = threadIdx.x;
    if (t < 2 * S3_NSIM) eg_perturb_one(sim3_load(t < S3_NSIM ? Si : Sj), t % S3_NSIM, fix_scale != 0, &s_pert[t / S3_NSIM][(t % S3_NSIM) * S3_SIM_STRIDE]);
    __syncthreads();
    if (t == 0) eg_edge_linearize(sim3_load(C), s_pert[0], s_pert[1], free_i != 0, free_j != 0, out);
}

__global__ __launch_bounds__(EG_THREADS) void assemble_kernel(const int32_t *plan, const double *eblk, double *H, double *b)
{
    const orbfe_essential_plan_header h = *(const orbfe_essential_plan_header *)plan;
    const int32_t *slot_ptr = plan + h.off_slot_ptr, *slot_edges = plan + h.off_slot_edges;
    const int n_slots = h.n_free + h.n_lblocks;
    for (int t = threadIdx.x; t < n_slots * 49; t += EG_THREADS) {
        const int s = t / 49, r = t - s * 49;
        H[t] = eg_slot_element(slot_edges, slot_ptr[s], slot_ptr[s + 1], s < h.n_free, eblk, r / 7, r % 7);
    }
    for (int t = threadIdx.x; t < h.n_free * 7; t += EG_THREADS) b[t] = eg_rhs_element(slot_edges, slot_ptr[t / 7], slot_ptr[t / 7 + 1], eblk, t % 7);
}

template <bool IN_LDS>
__global__ __launch_bounds__(EG_THREADS) void solve_kernel(const int32_t *plan, const double *H, const double *b, double lambda, double *F, double *x, int *ok)
{
    extern __shared__ double s_dyn[];
    __shared__ int s_fail;
    const orbfe_essential_plan_header h = *(const orbfe_essential_plan_header *)plan;
    EgPlan P;
    P.pos = plan + h.off_pos; P.colptr = plan + h.off_colptr; P.rowidx = plan + h.off_rowidx; P.slot_ptr = plan + h.off_slot_ptr;
    P.slot_edges = plan + h.off_slot_edges; P.upd_ptr = plan + h.off_upd_ptr; P.upd = plan + h.off_upd;
    P.n_free = h.n_free; P.n_slots = h.n_free + h.n_lblocks;
    double *W = IN_LDS ? s_dyn : F;
    const bool solved = eg_solve(H, b, P, lambda, W, &s_fail);
    for (int t = threadIdx.x; t < P.n_free * 7; t += EG_THREADS) x[t] = W[(size_t)P.n_slots * 49 + t];
    if (threadIdx.x == 0) *ok = solved ? 1 : 0;
}

__global__ void finish_kernel(int n, const double *S, float *T, float *Ow, int n_pts, const double *Srw, const double *Swr, float *pos)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) eg_recover_pose(sim3_load(S + 8 * (size_t)k), T + 16 * (size_t)k, Ow + 3 * (size_t)k);
    if (k < n_pts) eg_correct_point(sim3_load(Srw + 8 * (size_t)k), sim3_load(Swr + 8 * (size_t)k), pos + 3 * (size_t)k);
}

} // namespace

extern "C" int eb_log(int n, const double *S, double *out)
{
    if (n <= 0) return 0;
    Dev d;
    const double *dS = d.up(S, 8 * (size_t)n);
    double *dO = d.up<double>(nullptr, 7 * (size_t)n);
    if (!d.ok) return -1;
    hipLaunchKernelGGL(log_kernel, dim3((n + 63) / 64), dim3(64), 0, nullptr, n, dS, dO);
    d.down(out, dO, 7 * (size_t)n);
    return d.ok ? 0 : -1;
}

extern "C" int eb_edge(const double *C, const double *Si, const double *Sj, int free_i, int free_j, int fix_scale, double *out /*[105]*/)
{
    Dev d;
    const double *dC = d.up(C, 8), *dSi = d.up(Si, 8), *dSj = d.up(Sj, 8);
    double *dO = d.up<double>(nullptr, EG_EDGE_DOUBLES);
    if (!d.ok) return -1;
    hipLaunchKernelGGL(edge_kernel, dim3(1), dim3(64), 0, nullptr, dC, dSi, dSj, free_i, free_j, fix_scale, dO);
    d.down(out, dO, EG_EDGE_DOUBLES);
    return d.ok ? 0 : -1;
}

extern "C" int eb_assemble(const int32_t *plan, int plan_words, const double *eblk, int n_edges, double *H, double *b)
{
    orbfe_essential_plan_header h;
    memcpy(&h, plan, sizeof(h));
    if (h.magic != ORBFE_ESSENTIAL_PLAN_MAGIC || h.blob_bytes != plan_words * 4 || h.n_edges != n_edges) return -2;
    const size_t n_slots = (size_t)h.n_free + h.n_lblocks;
    Dev d;
    const int32_t *dP = d.up(plan, (size_t)plan_words);
    const double *dE = d.up(eblk, (size_t)EG_EDGE_DOUBLES * n_edges);
    double *dH = d.up<double>(nullptr, 49 * n_slots), *dB = d.up<double>(nullptr, 7 * (size_t)h.n_free);
    if (!d.ok) return -1;
    hipLaunchKernelGGL(assemble_kernel, dim3(1), dim3(EG_THREADS), 0, nullptr, dP, dE, dH, dB);
    d.down(H, dH, 49 * n_slots);
    d.down(b, dB, 7 * (size_t)h.n_free);
    return d.ok ? 0 : -1;
}

extern "C" int eb_solve(const int32_t *plan, int plan_words, const double *H, const double *b, double lambda, int in_lds, double *x, int *ok)
{
    orbfe_essential_plan_header h;
    memcpy(&h, plan, sizeof(h));
    if (h.magic != ORBFE_ESSENTIAL_PLAN_MAGIC || h.blob_bytes != plan_words * 4) return -2;
    const size_t n_slots = (size_t)h.n_free + h.n_lblocks, ws = 49 * n_slots + 7 * (size_t)h.n_free;
    if (in_lds && ws > (size_t)ORBFE_EG_LDS_DOUBLES) return -3;
    Dev d;
    const int32_t *dP = d.up(plan, (size_t)plan_words);
    const double *dH = d.up(H, 49 * n_slots), *dB = d.up(b, 7 * (size_t)h.n_free);
    double *dF = d.up<double>(nullptr, ws), *dX = d.up<double>(nullptr, 7 * (size_t)h.n_free);
    int *dOk = d.up<int>(nullptr, 1);
    if (!d.ok) return -1;
    if (in_lds) {
        if (hipFuncSetAttribute((const void *)solve_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(double) * ORBFE_EG_LDS_DOUBLES)) != hipSuccess) return -1;
        hipLaunchKernelGGL((solve_kernel<true>), dim3(1), dim3(EG_THREADS), sizeof(double) * (ws ? ws : 1), nullptr, dP, dH, dB, lambda, dF, dX, dOk);
    } else {
        hipLaunchKernelGGL((solve_kernel<false>), dim3(1), dim3(EG_THREADS), 8, nullptr, dP, dH, dB, lambda, dF, dX, dOk);
    }
    d.down(x, dX, 7 * (size_t)h.n_free);
    d.down(ok, dOk, 1);
    return d.ok ? 0 : -1;
}

extern "C" int eb_finish(int n, const double *S, float *T, float *Ow, int n_pts, const double *Srw, const double *Swr, float *pos)
{
    Dev d;
    const double *dS = d.up(S, 8 * (size_t)n), *dA = d.up(Srw, 8 * (size_t)n_pts), *dB = d.up(Swr, 8 * (size_t)n_pts);
    float *dT = d.up<float>(nullptr, 16 * (size_t)n), *dO = d.up<float>(nullptr, 3 * (size_t)n), *dPos = d.up(pos, 3 * (size_t)n_pts);
    if (!d.ok) return -1;
    const int m = n > n_pts ? n : n_pts;
    if (m <= 0) return 0;
    hipLaunchKernelGGL(finish_kernel, dim3((m + 63) / 64), dim3(64), 0, nullptr, n, dS, dT, dO, n_pts, dA, dB, dPos);
    d.down(T, dT, 16 * (size_t)n);
    d.down(Ow, dO, 3 * (size_t)n);
    d.down(pos, dPos, 3 * (size_t)n_pts);
    return d.ok ? 0 : -1;
}
