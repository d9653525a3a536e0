// orbfe_essential_graph.hip -- Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:825-1088) of LoopClosing::CorrectLoop on
// device-resident keyframes and the map-point table's position column, asynchronous on the caller's stream.  The edge walk of :891-1027
// stays the caller's and arrives as (i, j, kind); the symbolic work is the host planner's (orbfe_essential_plan.cpp), uploaded once.
//
// Launch 1: ONE workgroup of EG_THREADS threads runs the vertices, the measurements, optimize(iterations) with every Levenberg trial,
// and the recovery of the poses; the host does nothing in between.  FP64.  Every floating-point sum has an order fixed by the inputs:
//   per edge    its owner lane: e, Ji, Jj (numeric, central differences over the per-vertex table of 14 perturbed Sim3s)
//   per slot    49 lanes, one per element, walk the slot's edge list in the plan's order: no floating-point atomics
//   totals      eg_block_sum: the lanes' strided partials, then a fixed tree
//   per trial   F = H + lambda I, a right-looking block LDLT without pivoting along the plan.  Per pivot three barrier intervals: the
//               7 x 7 diagonal block in place (one lane, with the forward substitution of its right-hand side), the rows of the
//               column's blocks (one lane per row), the pivot's updates spread over the lanes (one lane per element, with the
//               right-hand side's).  Then the backward substitution, one interval per pivot.
// F and the right-hand side live in the LDS while they fit ORBFE_EG_LDS_DOUBLES, in the context's grow-only scratch above that;
// everything else (vertices, measurements, per-edge blocks, H) is scratch in HBM.
// Launch 2: one lane per point, any number of workgroups, no scratch of its own.
//
// g2o call map:  eg_evaluate                      = computeActiveErrors + activeChi2 (no robust kernel)
//                eg_linearize                     = linearizeOplus + constructQuadraticForm of every edge (BlockSolver::buildSystem)
//                eg_solve                         = setLambda + BlockSolver::solve with LinearSolverEigen (a sparse LDLT), restoreDiagonal
//                the do/while, the for            = OptimizationAlgorithmLevenberg::solve, SparseOptimizer::optimize (section 4a)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "orbfe_device.h"
#include "orbfe_host.h"

#include "orbfe_essential_blocks.hpp"

#pragma clang fp contract(off)

namespace {

constexpr size_t EG_LDS_REQUEST = 128 * 1024; // of the CU's 160 KiB, as the bundle adjustment
constexpr size_t EG_FIXED_BYTES = 2560;       // the kernel's static LDS: the reduction's partials and a few flags
static_assert(sizeof(double) * EG_THREADS + 64 <= EG_FIXED_BYTES, "the static part fits its share");
static_assert((size_t)ORBFE_EG_LDS_DOUBLES == (EG_LDS_REQUEST - EG_FIXED_BYTES) / sizeof(double), "the cap is derived from the request, not chosen");

struct EgArgs {
    float *Tcw;
    const double *corr, *nonc;
    const uint8_t *has_corr, *has_nonc, *ekind;
    const int32_t *ei, *ej, *plan;
    orbfe_obs_keyframe *obs_kfs;
    uint8_t *edge_code;
    double *sim3_out;
    orbfe_essential_graph_info *info;
    int32_t *status;
    // scratch
    double *init, *est[2], *invf, *meas, *pert, *eblk, *H, *b, *x, *F;
    uint8_t *vbad;
    int32_t n_kfs, fixed_kf, n_edges, n_lblocks, plan_bytes, iterations, fix_scale;
    double lambda_init;
};

struct EgPointArgs {
    const int32_t *plan, *pt_ref;
    const uint8_t *pt_valid, *vbad;
    const double *init, *invf;
    float *pos;
    uint8_t *pt_code;
    int32_t *status;
    int32_t n_kfs, fixed_kf, n_edges, n_lblocks, plan_bytes, n_pts;
};

__host__ __device__ inline size_t eg_workspace_doubles(int n_free, int n_lblocks) { return ((size_t)n_free + (size_t)n_lblocks) * 49 + (size_t)n_free * 7; }

// the scratch of one call, carved from one buffer; base == nullptr: only the size
size_t eg_carve(EgArgs &a, uint8_t *base, bool workspace_in_hbm)
{
    const size_t K = (size_t)std::max(a.n_kfs, 1), E = (size_t)std::max(a.n_edges, 1), n_free = K - 1, S = n_free + (size_t)a.n_lblocks;
    orbfe::Arena c(base, sizeof(double), sizeof(double)); // an empty field still holds one double
    a.init = c.take<double>(8 * K); a.est[0] = c.take<double>(8 * K); a.est[1] = c.take<double>(8 * K); a.invf = c.take<double>(8 * K); a.meas = c.take<double>(8 * E);
    a.pert = c.take<double>((size_t)EG_PERT_STRIDE * K); a.eblk = c.take<double>((size_t)EG_EDGE_DOUBLES * E); a.H = c.take<double>(49 * S);
    a.b = c.take<double>(7 * n_free); a.x = c.take<double>(7 * n_free);
    a.F = workspace_in_hbm ? c.take<double>(eg_workspace_doubles((int)n_free, a.n_lblocks)) : nullptr; a.vbad = c.take<uint8_t>(orbfe::round_up(K, 16));
    return c.bytes();
}

// the device header against the call's arguments, and the sections against the header: after this every section lies inside the blob
__device__ inline bool eg_plan_matches(const int32_t *plan, int n_kfs, int fixed_kf, int n_edges, int n_lblocks, int plan_bytes)
{
    const orbfe_essential_plan_header h = *(const orbfe_essential_plan_header *)plan;
    if (h.magic != ORBFE_ESSENTIAL_PLAN_MAGIC || h.n_kfs != n_kfs || h.fixed_kf != fixed_kf || h.n_edges != n_edges || h.n_lblocks != n_lblocks ||
        h.blob_bytes != plan_bytes || h.n_free != n_kfs - 1 || h.n_slot_edges < 0 || h.n_updates < 0)
        return false;
    long long at = sizeof(orbfe_essential_plan_header) / 4;
    const long long n_free = h.n_free, n_slots = n_free + n_lblocks;
    const long long sizes[9] = {n_free, n_kfs, n_free + 1, n_lblocks, 4ll * n_edges, n_slots + 1, h.n_slot_edges, n_free + 1, 3ll * h.n_updates};
    const int32_t offs[9] = {h.off_order, h.off_pos, h.off_colptr, h.off_rowidx, h.off_edge_slots, h.off_slot_ptr, h.off_slot_edges, h.off_upd_ptr, h.off_upd};
    for (int k = 0; k < 9; k++) {
        if ((long long)offs[k] != at) return false;
        at += sizes[k];
    }
    return at * 4 == (long long)plan_bytes;
}

// chi2 = the sum of e.e over the edges that take part, at `est`
__device__ double eg_evaluate(const EgArgs &a, const double *est, double *s_red)
{
    double chi = 0.0;
    for (int e = threadIdx.x; e < a.n_edges; e += EG_THREADS) {
        if (a.edge_code[e]) continue;
        double err[7];
        eg_edge_error(sim3_load(a.meas + 8 * (size_t)e), sim3_load(est + 8 * (size_t)a.ei[e]), eg_inverse(sim3_load(est + 8 * (size_t)a.ej[e])), err);
        double c = 0.0;
#pragma unroll
        for (int k = 0; k < 7; k++) c += err[k] * err[k];
        chi += c;
    }
    return eg_block_sum(chi, s_red);
}

// H, b and chi2 at `est`
__device__ double eg_linearize(const EgArgs &a, const EgPlan &P, const double *est, double *s_red)
{
    for (int t = threadIdx.x; t < a.n_kfs * S3_NSIM; t += EG_THREADS) {
        const int v = t / S3_NSIM;
        if (!a.vbad[v]) eg_perturb_one(sim3_load(est + 8 * (size_t)v), t - v * S3_NSIM, a.fix_scale != 0, a.pert + (size_t)t * S3_SIM_STRIDE);
    }
    __syncthreads();
    double chi = 0.0;
    for (int e = threadIdx.x; e < a.n_edges; e += EG_THREADS) {
        double *out = a.eblk + (size_t)e * EG_EDGE_DOUBLES;
        if (a.edge_code[e]) {
            for (int k = 0; k < EG_EDGE_DOUBLES; k++) out[k] = 0.0; // an edge left out adds exact zeros to its slots
            continue;
        }
        const int i = a.ei[e], j = a.ej[e];
        eg_edge_linearize(sim3_load(a.meas + 8 * (size_t)e), a.pert + (size_t)i * EG_PERT_STRIDE, a.pert + (size_t)j * EG_PERT_STRIDE, i != a.fixed_kf,
                          j != a.fixed_kf, out);
        double c = 0.0;
#pragma unroll
        for (int k = 0; k < 7; k++) c += out[k] * out[k];
        chi += c;
    }
    chi = eg_block_sum(chi, s_red); // its barriers also publish the edge blocks
    for (int t = threadIdx.x; t < P.n_slots * 49; t += EG_THREADS) {
        const int s = t / 49, r = t - s * 49;
        a.H[t] = eg_slot_element(P.slot_edges, P.slot_ptr[s], P.slot_ptr[s + 1], s < P.n_free, a.eblk, r / 7, r % 7);
    }
    for (int t = threadIdx.x; t < P.n_free * 7; t += EG_THREADS) {
        const int p = t / 7;
        a.b[t] = eg_rhs_element(P.slot_edges, P.slot_ptr[p], P.slot_ptr[p + 1], a.eblk, t - p * 7);
    }
    __syncthreads();
    return chi;
}

template <bool IN_LDS>
__global__ __launch_bounds__(EG_THREADS) void eg_kernel(const EgArgs a)
{
    extern __shared__ double s_dyn[];
    __shared__ double s_red[EG_THREADS];
    __shared__ int s_flag[4]; // 0: a faulty edge or Sim3, 1: the factorisation failed, 2: edges that take part
    const int tid = threadIdx.x;
    if (!eg_plan_matches(a.plan, a.n_kfs, a.fixed_kf, a.n_edges, a.n_lblocks, a.plan_bytes)) { // the same in every lane
        if (tid == 0) *a.status = ORBFE_ERR_INVALID;
        return;
    }
    const orbfe_essential_plan_header h = *(const orbfe_essential_plan_header *)a.plan;
    EgPlan P;
    P.pos = a.plan + h.off_pos; P.colptr = a.plan + h.off_colptr; P.rowidx = a.plan + h.off_rowidx; P.slot_ptr = a.plan + h.off_slot_ptr;
    P.slot_edges = a.plan + h.off_slot_edges; P.upd_ptr = a.plan + h.off_upd_ptr; P.upd = a.plan + h.off_upd;
    P.n_free = h.n_free; P.n_slots = h.n_free + h.n_lblocks;
    double *F = IN_LDS ? s_dyn : a.F;
    if (tid < 4) s_flag[tid] = 0;
    __syncthreads();

    // ---- vertices (:853-888): vScw, the initial estimate
    for (int v = tid; v < a.n_kfs; v += EG_THREADS) {
        const Sim3D S = (a.has_corr && a.has_corr[v]) ? sim3_load(a.corr + 8 * (size_t)v) : eg_sim3_from_Tcw(a.Tcw + 16 * (size_t)v);
        const bool bad = !eg_sim3_finite(S);
        a.vbad[v] = bad ? 1 : 0;
        if (bad) s_flag[0] = 1; // every lane that writes writes this value
        sim3_store(S, a.init + 8 * (size_t)v);
        sim3_store(S, a.est[0] + 8 * (size_t)v);
        sim3_store(S, a.est[1] + 8 * (size_t)v);
    }
    for (int t = tid; t < P.n_free * 7; t += EG_THREADS) a.x[t] = 0.0;
    __syncthreads();
    // ---- measurements (:896-1027), formed once
    int mine = 0;
    for (int e = tid; e < a.n_edges; e += EG_THREADS) {
        const int i = a.ei[e], j = a.ej[e];
        int code = 0;
        if (i < 0 || i >= a.n_kfs || j < 0 || j >= a.n_kfs || i == j) code = ORBFE_EG_EDGE_INDEX; // checked before they become addresses
        else {
            const bool nc = a.ekind[e] != 0 && a.has_nonc != nullptr;
            const Sim3D Si = (nc && a.has_nonc[i]) ? sim3_load(a.nonc + 8 * (size_t)i) : sim3_load(a.init + 8 * (size_t)i);
            const Sim3D Sj = (nc && a.has_nonc[j]) ? sim3_load(a.nonc + 8 * (size_t)j) : sim3_load(a.init + 8 * (size_t)j);
            if (a.vbad[i] || a.vbad[j] || !eg_sim3_finite(Si) || !eg_sim3_finite(Sj)) code = ORBFE_EG_EDGE_SIM3;
            else sim3_store(eg_mul(Sj, eg_inverse(Si)), a.meas + 8 * (size_t)e);
        }
        a.edge_code[e] = (uint8_t)code;
        if (code) s_flag[0] = 1;
        else mine++;
    }
    if (mine) atomicAdd(&s_flag[2], mine); // an integer count: the order does not matter
    __syncthreads();
    const int n_active = s_flag[2];

    // ---- optimize(iterations): SparseOptimizer::optimize with OptimizationAlgorithmLevenberg (section 4a)
    int cur = 0, iterations = 0, trials = 0;
    double chi_start = 0.0, current_chi = 0.0, lambda = a.lambda_init;
    if (n_active > 0 && P.n_free > 0) { // otherwise no vertex is active and optimize() returns at once
        double ni = 2.0;
        int lm_bad = 0;
        const double *xv = F + (size_t)P.n_slots * 49;
        for (int it = 0; it < a.iterations; it++) {
            iterations++;
            const double *est = a.est[cur];
            double *trial = a.est[cur ^ 1];
            const double chi_here = eg_linearize(a, P, est, s_red);
            if (it == 0) { chi_start = chi_here; lambda = a.lambda_init; ni = 2.0; lm_bad = 0; } // computeLambdaInit: the user's value, > 0
            current_chi = chi_here;
            const double ini_chi = current_chi;
            double rho = 0.0;
            int qmax = 0;
            bool accepted = false;
            do {
                const bool ok2 = eg_solve(a.H, a.b, P, lambda, F, &s_flag[1]);
                double sc = 0.0; // computeScale(): a failed solve leaves the x of the solve before it, as LinearSolverEigen does
                for (int t = tid; t < P.n_free * 7; t += EG_THREADS) {
                    if (ok2) a.x[t] = xv[t];
                    sc += a.x[t] * (lambda * a.x[t] + a.b[t]);
                }
                double scale = eg_block_sum(sc, s_red);
                scale += 1e-3;
                double temp_chi = DBL_MAX;
                if (ok2) { // a failed factorisation is a rejected trial: nothing is updated
                    for (int v = tid; v < a.n_kfs; v += EG_THREADS) {
                        const Sim3D S = sim3_load(est + 8 * (size_t)v);
                        const int p = P.pos[v];
                        sim3_store((p >= 0 && !a.vbad[v]) ? sim3_oplus(xv + 7 * (size_t)p, a.fix_scale != 0, S) : S, trial + 8 * (size_t)v);
                    }
                    __syncthreads();
                    temp_chi = eg_evaluate(a, trial, s_red);
                }
                trials++;
                rho = (current_chi - temp_chi) / scale;
                if (rho > 0 && isfinite(temp_chi)) {
                    const double r21 = 2 * rho - 1;
                    double alpha = 1.0 - r21 * r21 * r21;
                    alpha = fmin(alpha, 2.0 / 3.0);
                    lambda *= fmax(1.0 / 3.0, alpha);
                    ni = 2;
                    current_chi = temp_chi;
                    accepted = ok2;
                } else {
                    lambda *= ni;
                    ni *= 2;
                }
                qmax++;
            } while (rho < 0 && qmax < 10);
            if (accepted) cur ^= 1;
            if (qmax == 10 || rho == 0) break;
            if ((ini_chi - current_chi) * 1e3 < ini_chi) lm_bad++;
            else lm_bad = 0;
            if (lm_bad >= 3) break;
        }
    }

    // ---- recovery (:1036-1054): every keyframe, the fixed one included
    const double *fin = a.est[cur];
    for (int v = tid; v < a.n_kfs; v += EG_THREADS) {
        const Sim3D S = sim3_load(fin + 8 * (size_t)v);
        if (a.sim3_out) sim3_store(S, a.sim3_out + 8 * (size_t)v);
        if (a.vbad[v]) continue;
        sim3_store(eg_inverse(S), a.invf + 8 * (size_t)v);
        float T[16], Ow[3];
        eg_recover_pose(S, T, Ow);
#pragma unroll
        for (int i = 0; i < 16; i++) a.Tcw[16 * (size_t)v + i] = T[i];
        if (a.obs_kfs) {
#pragma unroll
            for (int i = 0; i < 3; i++) a.obs_kfs[v].Ow[i] = Ow[i];
        }
    }
    if (tid == 0) {
        orbfe_essential_graph_info o = {};
        o.iterations = iterations; o.trials = trials; o.n_active_edges = n_active; o.n_lblocks = a.n_lblocks;
        o.chi2_start = chi_start; o.chi2_end = current_chi; o.lambda_last = lambda; o.in_lds = IN_LDS ? 1 : 0;
        *a.info = o;
        *a.status = s_flag[0] ? ORBFE_ERR_INVALID : 0;
    }
}

// ---- points (:1057-1087): correctedSwr.map(Srw.map(pos)), Srw the INITIAL estimate of the point's keyframe
__global__ __launch_bounds__(EG_THREADS) void eg_points_kernel(const EgPointArgs a)
{
    if (!eg_plan_matches(a.plan, a.n_kfs, a.fixed_kf, a.n_edges, a.n_lblocks, a.plan_bytes)) return; // launch 1 has said so
    const int q = blockIdx.x * EG_THREADS + threadIdx.x;
    if (q >= a.n_pts) return;
    int code = 0;
    if (a.pt_valid[q]) {
        const int r = a.pt_ref[q];
        if (r < 0 || r >= a.n_kfs) { code = 1; *a.status = ORBFE_ERR_INVALID; } // checked before it becomes an address
        else if (!a.vbad[r]) {
            float p[3] = {a.pos[3 * (size_t)q], a.pos[3 * (size_t)q + 1], a.pos[3 * (size_t)q + 2]};
            eg_correct_point(sim3_load(a.init + 8 * (size_t)r), sim3_load(a.invf + 8 * (size_t)r), p);
            a.pos[3 * (size_t)q] = p[0]; a.pos[3 * (size_t)q + 1] = p[1]; a.pos[3 * (size_t)q + 2] = p[2];
        }
    }
    if (a.pt_code) a.pt_code[q] = (uint8_t)code;
}

} // namespace

extern "C" int orbfe_enqueue_optimize_essential_graph(orbfe_context *ctx, int n_kfs, int fixed_kf, float *d_Tcw, const double *d_corrected,
                                                      const uint8_t *d_has_corrected, const double *d_noncorrected, const uint8_t *d_has_noncorrected,
                                                      const int32_t *d_edge_i, const int32_t *d_edge_j, const uint8_t *d_edge_kind, int n_edges,
                                                      const void *d_plan, const orbfe_essential_plan_header *h_plan_header, int iterations, int fix_scale,
                                                      double lambda_init, float *d_pos, const int32_t *d_pt_ref, const uint8_t *d_pt_valid, int n_pts,
                                                      orbfe_obs_keyframe *d_obs_kfs, uint8_t *d_edge_code, uint8_t *d_pt_code, double *d_sim3_out,
                                                      orbfe_essential_graph_info *d_info, int32_t *d_status, void *stream)
try {
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    ORBFE_ENTRY(ctx);
    if (!d_Tcw || !d_plan || !h_plan_header || !d_info || !d_status) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null argument");
    if (n_kfs < 1 || n_edges < 0 || n_pts < 0 || iterations < 0) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "n_kfs = %d, n_edges = %d, n_pts = %d, iterations = %d", n_kfs, n_edges, n_pts, iterations);
    if (fixed_kf < 0 || fixed_kf >= n_kfs) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "fixed_kf = %d outside [0, %d)", fixed_kf, n_kfs);
    if (!(lambda_init > 0)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "lambda_init must be > 0");
    if (n_edges > 0 && (!d_edge_i || !d_edge_j || !d_edge_kind || !d_edge_code)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null edge array");
    if (n_pts > 0 && (!d_pos || !d_pt_ref || !d_pt_valid)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null point array");
    if ((d_corrected == nullptr) != (d_has_corrected == nullptr) || (d_noncorrected == nullptr) != (d_has_noncorrected == nullptr))
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "a Sim3 table and its flags come together");
    const int n_lblocks = h_plan_header->n_lblocks, plan_bytes = h_plan_header->blob_bytes;
    if (n_lblocks < 0 || plan_bytes < (int)sizeof(orbfe_essential_plan_header)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "not a plan header");
    hipStream_t s;
    if (const int rc = orbfe_enqueue_on(ctx, stream, false, &s)) return rc;
    EgArgs a = {};
    a.Tcw = d_Tcw; a.corr = d_corrected; a.has_corr = d_has_corrected; a.nonc = d_noncorrected; a.has_nonc = d_has_noncorrected;
    a.ei = d_edge_i; a.ej = d_edge_j; a.ekind = d_edge_kind; a.plan = (const int32_t *)d_plan; a.obs_kfs = d_obs_kfs; a.edge_code = d_edge_code;
    a.sim3_out = d_sim3_out; a.info = d_info; a.status = d_status;
    a.n_kfs = n_kfs; a.fixed_kf = fixed_kf; a.n_edges = n_edges; a.n_lblocks = n_lblocks; a.plan_bytes = plan_bytes; a.iterations = iterations;
    a.fix_scale = fix_scale ? 1 : 0; a.lambda_init = lambda_init;
    const size_t ws = eg_workspace_doubles(n_kfs - 1, n_lblocks);
    const bool in_lds = ws <= (size_t)ORBFE_EG_LDS_DOUBLES;
    const size_t bytes = eg_carve(a, nullptr, !in_lds);
    if (ctx->eg_scratch.ensure(bytes)) return orbfe_fail(ctx, ORBFE_ERR_HIP, "essential graph scratch allocation of %zu bytes failed", bytes);
    eg_carve(a, (uint8_t *)ctx->eg_scratch.p, !in_lds);
    if (in_lds) {
        ORBFE_HIP_TRY(ctx, hipFuncSetAttribute((const void *)eg_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(EG_LDS_REQUEST - EG_FIXED_BYTES)));
        hipLaunchKernelGGL((eg_kernel<true>), dim3(1), dim3(EG_THREADS), std::max<size_t>(ws * sizeof(double), 8), s, a);
    } else {
        hipLaunchKernelGGL((eg_kernel<false>), dim3(1), dim3(EG_THREADS), 8, s, a);
    }
    ORBFE_HIP_TRY(ctx, hipGetLastError());
    if (n_pts > 0) {
        EgPointArgs p = {};
        p.plan = a.plan; p.pt_ref = d_pt_ref; p.pt_valid = d_pt_valid; p.vbad = a.vbad; p.init = a.init; p.invf = a.invf; p.pos = d_pos; p.pt_code = d_pt_code;
        p.status = d_status; p.n_kfs = n_kfs; p.fixed_kf = fixed_kf; p.n_edges = n_edges; p.n_lblocks = n_lblocks; p.plan_bytes = plan_bytes; p.n_pts = n_pts;
        hipLaunchKernelGGL(eg_points_kernel, dim3((unsigned)((n_pts + EG_THREADS - 1) / EG_THREADS)), dim3(EG_THREADS), 0, s, p);
        ORBFE_HIP_TRY(ctx, hipGetLastError());
    }
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

extern "C" int orbfe_optimize_essential_graph(orbfe_context *ctx, int n_kfs, int fixed_kf, float *Tcw, const double *corrected, const uint8_t *has_corrected,
                                              const double *noncorrected, const uint8_t *has_noncorrected, const int32_t *edge_i, const int32_t *edge_j,
                                              const uint8_t *edge_kind, int n_edges, int iterations, int fix_scale, double lambda_init, float *pos,
                                              const int32_t *pt_ref, const uint8_t *pt_valid, int n_pts, float *Ow, uint8_t *edge_code, uint8_t *pt_code,
                                              double *sim3_out, orbfe_essential_graph_info *info, int32_t *status)
try {
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    ORBFE_ENTRY(ctx);
    if (!Tcw || !info || !status) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null argument");
    if (n_kfs < 1 || n_edges < 0 || n_pts < 0) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "n_kfs = %d, n_edges = %d, n_pts = %d", n_kfs, n_edges, n_pts);
    if (n_edges > 0 && (!edge_i || !edge_j || !edge_kind || !edge_code)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null edge array");
    if (n_pts > 0 && (!pos || !pt_ref || !pt_valid)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null point array");
    if ((corrected == nullptr) != (has_corrected == nullptr) || (noncorrected == nullptr) != (has_noncorrected == nullptr))
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "a Sim3 table and its flags come together");
    size_t plan_bytes = 0;
    int rc = orbfe_essential_graph_plan_size(n_kfs, fixed_kf, edge_i, edge_j, n_edges, &plan_bytes);
    if (rc != ORBFE_OK) return orbfe_fail(ctx, rc, "the planner refused the graph (n_kfs = %d, fixed_kf = %d, n_edges = %d)", n_kfs, fixed_kf, n_edges);
    hipStream_t s;
    if ((rc = orbfe_enqueue_on(ctx, nullptr, false, &s))) return rc;
    // the staging block: results first, then the inputs; the planner writes its blob straight into the host image
    const size_t K = (size_t)n_kfs;
    orbfe::StageLayout L;
    const auto f_info = L.result<orbfe_essential_graph_info>(1); const auto f_status = L.result<int32_t>(1); const auto f_T = L.result<float>(K, 16);
    const auto f_pos = L.result<float>(n_pts, 3); const auto f_okf = L.result<orbfe_obs_keyframe>(K); const auto f_sim = L.result<double>(K, 8);
    const auto f_ecode = L.result<uint8_t>(n_edges); const auto f_pcode = L.result<uint8_t>(n_pts);
    const auto f_corr = L.input<double>(K, 8);
    const auto f_hc = L.input<uint8_t>(K); const auto f_nonc = L.input<double>(K, 8); const auto f_hn = L.input<uint8_t>(K);
    const auto f_ei = L.input<int32_t>(n_edges); const auto f_ej = L.input<int32_t>(n_edges); const auto f_kind = L.input<uint8_t>(n_edges);
    const auto f_ref = L.input<int32_t>(n_pts); const auto f_valid = L.input<uint8_t>(n_pts); const auto f_plan = L.input<uint8_t>(plan_bytes);
    if (ctx->sync_stage.ensure(L.bytes())) return orbfe_fail(ctx, ORBFE_ERR_HIP, "essential graph staging allocation failed");
    StageBlock blk(L, ctx->sync_stage);
    blk.put(f_T, Tcw, 16 * K); blk.put(f_pos, pos, 3 * (size_t)n_pts); blk.put(f_ref, pt_ref, n_pts); blk.put(f_valid, pt_valid, n_pts);
    if (corrected) { blk.put(f_corr, corrected, 8 * K); blk.put(f_hc, has_corrected, K); }
    if (noncorrected) { blk.put(f_nonc, noncorrected, 8 * K); blk.put(f_hn, has_noncorrected, K); }
    blk.put(f_ei, edge_i, n_edges); blk.put(f_ej, edge_j, n_edges); blk.put(f_kind, edge_kind, n_edges);
    size_t got = 0;
    rc = orbfe_essential_graph_plan(n_kfs, fixed_kf, edge_i, edge_j, n_edges, blk.host(f_plan), f_plan.count, &got);
    if (rc != ORBFE_OK) return orbfe_fail(ctx, rc, "the planner refused the graph");
    orbfe_essential_plan_header hdr;
    memcpy(&hdr, blk.host(f_plan), sizeof(hdr));
    ORBFE_HIP_TRY(ctx, blk.upload(s));
    rc = orbfe_enqueue_optimize_essential_graph(ctx, n_kfs, fixed_kf, blk.dev(f_T), corrected ? blk.dev(f_corr) : nullptr, corrected ? blk.dev(f_hc) : nullptr,
                                                noncorrected ? blk.dev(f_nonc) : nullptr, noncorrected ? blk.dev(f_hn) : nullptr, blk.dev(f_ei), blk.dev(f_ej),
                                                blk.dev(f_kind), n_edges, blk.dev(f_plan), &hdr, iterations, fix_scale, lambda_init, blk.dev(f_pos), blk.dev(f_ref),
                                                blk.dev(f_valid), n_pts, Ow ? blk.dev(f_okf) : nullptr, blk.dev(f_ecode), blk.dev(f_pcode), blk.dev(f_sim),
                                                blk.dev(f_info), blk.dev(f_status), nullptr);
    if (rc != ORBFE_OK) return rc;
    ORBFE_HIP_TRY(ctx, blk.download(s));
    ORBFE_HIP_TRY(ctx, hipStreamSynchronize(s));
    blk.get(f_info, info, 1); blk.get(f_status, status, 1); blk.get(f_T, Tcw, 16 * K); blk.get(f_pos, pos, 3 * (size_t)n_pts);
    if (Ow) {
        const orbfe_obs_keyframe *okf = blk.host(f_okf);
        for (size_t k = 0; k < K; k++) memcpy(Ow + 3 * k, okf[k].Ow, sizeof(float) * 3);
    }
    if (sim3_out) blk.get(f_sim, sim3_out, 8 * K);
    blk.get(f_ecode, edge_code, n_edges);
    if (pt_code) blk.get(f_pcode, pt_code, n_pts);
    return ORBFE_OK;
} ORBFE_CATCH(ctx)
