// orbfe_sim3_blocks.hpp -- the device building blocks of orbfe_sim3_opt.hip (g2o's Sim3 algebra, the two projection errors of
// Optimizer::OptimizeSim3 with BaseBinaryEdge's numeric Jacobian, the compacted correspondence table and the evaluation pass), in a
// header so that a test-only translation unit (tests/sim3_blocks/sim3_blocks.hip) can run each of them alone against the float64 model
// (tests/sim3_opt_model.py).  The 7 x 7 solve is solve_ldlt<7> of orbfe_pose_blocks.hpp.  Device code only.
//
// g2o call map:  sim3_from_rts            = Sim3(Matrix3d, Vector3d, double)            (types/sim3.h:64-67; Quaterniond(R), NOT normalised)
//                sim3_exp                 = Sim3(Vector7d)                              (:70-142, the four (|sigma|, theta) < 1e-5 branches)
//                sim3_map / _mul / _inverse = map, operator*, inverse                   (:144-146, :266-272, :233-236)
//                sim3_oplus               = VertexSim3Expmap::oplusImpl                 (types/types_seven_dof_expmap.h:60-69)
//                sim3_edge_error          = EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ::computeError (:138-145, :160-167)
//                sim3_perturb             = the 14 oplus calls of BaseBinaryEdge::linearizeOplus (core/base_binary_edge.hpp:176-197),
//                                           which do not depend on the edge: formed once per pass, with their inverses
//                sim3_eval_pass           = computeActiveErrors + activeRobustChi2 + linearizeOplus + constructQuadraticForm (:91-113)
#pragma once
#include "orbfe_pose_blocks.hpp" // Se3, quat_from_matrix, quat_rotate, dpp_f64, row_transpose_step, solve_ldlt, and the FP64 contract

// FP64 throughout like g2o, compared with a tolerance: fused multiply-adds are allowed, as in orbfe_pose_blocks.hpp.
#pragma clang fp contract(fast)

namespace {

struct Sim3D { Se3 q; double s; }; // q.x q.y q.z q.w (any norm: g2o never normalises it), q.t, scale
struct CamK { double fx, fy, cx, cy; };

constexpr int S3_NVAL = 40;   // values one pass sums: H (28, upper triangle row-major), b (7), robust chi2, #active, 3 unused
constexpr int S3_NSIM = 15;   // Sim3s one pass evaluates: +delta / -delta per dimension, then the estimate itself
constexpr int S3_SIM_STRIDE = 16; // doubles per entry of the pass's Sim3 list: S (8), S.inverse() (8)
constexpr int S3_CHI = 35, S3_CNT = 36;

__device__ inline Sim3D sim3_from_rts(const double R[3][3], const double t[3], double s)
{
    Sim3D S;
    quat_from_matrix(R, S.q);
    S.q.t[0] = t[0]; S.q.t[1] = t[1]; S.q.t[2] = t[2];
    S.s = s;
    return S;
}

__device__ inline void sim3_map(const Sim3D &S, const double p[3], double out[3])
{
    double r[3];
    quat_rotate(S.q, p, r);
#pragma unroll
    for (int i = 0; i < 3; i++) out[i] = S.s * r[i] + S.q.t[i];
}

__device__ inline Sim3D sim3_mul(const Sim3D &a, const Sim3D &b)
{
    Sim3D r;
    double rt[3];
    quat_rotate(a.q, b.q.t, rt);
#pragma unroll
    for (int i = 0; i < 3; i++) r.q.t[i] = a.s * rt[i] + a.q.t[i];
    r.q.w = a.q.w * b.q.w - a.q.x * b.q.x - a.q.y * b.q.y - a.q.z * b.q.z;
    r.q.x = a.q.w * b.q.x + a.q.x * b.q.w + a.q.y * b.q.z - a.q.z * b.q.y;
    r.q.y = a.q.w * b.q.y + a.q.y * b.q.w + a.q.z * b.q.x - a.q.x * b.q.z;
    r.q.z = a.q.w * b.q.z + a.q.z * b.q.w + a.q.x * b.q.y - a.q.y * b.q.x;
    r.s = a.s * b.s;
    return r;
}

__device__ inline Sim3D sim3_inverse(const Sim3D &a)
{
    Sim3D r;
    r.q.x = -a.q.x; r.q.y = -a.q.y; r.q.z = -a.q.z; r.q.w = a.q.w;
    const double k = -1. / a.s;
    const double v[3] = {k * a.q.t[0], k * a.q.t[1], k * a.q.t[2]};
    quat_rotate(r.q, v, r.q.t);
    r.s = 1. / a.s;
    return r;
}

__device__ inline Sim3D sim3_exp(const double u[7])
{
    const double om[3] = {u[0], u[1], u[2]};
    const double sigma = u[6];
    const double theta = sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);
    const double O[3][3] = {{0, -om[2], om[1]}, {om[2], 0, -om[0]}, {-om[1], om[0], 0}};
    double O2[3][3], R[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double s = 0;
#pragma unroll
            for (int k = 0; k < 3; k++) s += O[i][k] * O[k][j];
            O2[i][j] = s;
        }
    const double s = exp(sigma);
    const double eps = 0.00001;
    const bool small_theta = theta < eps;
    double A, B, C;
    double ra = 1.0, rb = 1.0; // R = I + ra Omega + rb Omega^2; theta < eps: I + Omega + Omega^2, not orthonormal
    if (!small_theta) {
        ra = sin(theta) / theta;
        rb = (1 - cos(theta)) / (theta * theta);
    }
    if (fabs(sigma) < eps) {
        C = 1;
        if (small_theta) {
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta2 = theta * theta;
            A = (1 - cos(theta)) / theta2;
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (s - 1) / sigma;
        if (small_theta) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
        } else {
            const double a = s * sin(theta), b = s * cos(theta);
            const double theta2 = theta * theta, sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    }
    double t[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        double acc = 0;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double id = (i == j) ? 1.0 : 0.0;
            R[i][j] = id + ra * O[i][j] + rb * O2[i][j];
            acc += (A * O[i][j] + B * O2[i][j] + C * id) * u[3 + j];
        }
        t[i] = acc;
    }
    return sim3_from_rts(R, t, s);
}

// VertexSim3Expmap::oplusImpl: estimate <- Sim3(update) * estimate, with update[6] = 0 under _fix_scale
__device__ inline Sim3D sim3_oplus(const double upd[7], bool fix_scale, const Sim3D &est)
{
    double u[7];
#pragma unroll
    for (int j = 0; j < 7; j++) u[j] = upd[j];
    if (fix_scale) u[6] = 0;
    return sim3_mul(sim3_exp(u), est);
}

__device__ __forceinline__ void sim3_store(const Sim3D &S, double *p)
{
    p[0] = S.q.x; p[1] = S.q.y; p[2] = S.q.z; p[3] = S.q.w; p[4] = S.q.t[0]; p[5] = S.q.t[1]; p[6] = S.q.t[2]; p[7] = S.s;
}
__device__ __forceinline__ Sim3D sim3_load(const double *p)
{
    Sim3D S;
    S.q.x = p[0]; S.q.y = p[1]; S.q.z = p[2]; S.q.w = p[3]; S.q.t[0] = p[4]; S.q.t[1] = p[5]; S.q.t[2] = p[6]; S.s = p[7];
    return S;
}

// obs - cam_map(project(S.map(P))): the error of either edge class (the inverse edge passes S.inverse())
__device__ __forceinline__ void sim3_edge_error(const Sim3D &S, const CamK &c, const double P[3], const double obs[2], double e[2])
{
    double p[3];
    sim3_map(S, P, p);
    e[0] = obs[0] - (p[0] / p[2] * c.fx + c.cx);
    e[1] = obs[1] - (p[1] / p[2] * c.fy + c.cy);
}

// RobustKernelHuber::robustify (core/robust_kernel_impl.cpp:78-91): rho[0], rho[1]
__device__ __forceinline__ void huber(double e2, double delta, double &rho0, double &rho1)
{
    const double dsqr = delta * delta;
    if (e2 <= dsqr) { rho0 = e2; rho1 = 1.; }
    else {
        const double sqrte = sqrt(e2);
        rho0 = 2 * sqrte * delta - dsqr;
        rho1 = delta / sqrte;
    }
}

// The Sim3s of one pass at `est`, written by the first 15 threads and followed by a barrier: entry 2 d + (0: +delta, 1: -delta) is
// oplus(+-1e-9 along dimension d), entry 14 the estimate; each with its inverse.  Under fix_scale entries 12 and 13 are oplus(0) = the
// estimate, bit for bit (Sim3(0) is the identity and 1 * x + 0 is exact), so column 6 of every Jacobian is exactly zero.
__device__ inline void sim3_perturb(const Sim3D &est, bool fix_scale, double *s_sims /*[S3_NSIM][S3_SIM_STRIDE]*/)
{
    const int k = threadIdx.x;
    if (k < S3_NSIM) {
        Sim3D S = est;
        if (k < S3_NSIM - 1) {
            const double delta = 1e-9;
            double u[7];
#pragma unroll
            for (int j = 0; j < 7; j++) u[j] = (j == (k >> 1)) ? ((k & 1) ? -delta : delta) : 0.0;
            S = sim3_oplus(u, fix_scale, est);
        }
        sim3_store(S, s_sims + k * S3_SIM_STRIDE);
        sim3_store(sim3_inverse(S), s_sims + k * S3_SIM_STRIDE + 8);
    }
    __syncthreads();
}

// The compacted correspondences of one call, in ascending keypoint slot of KF1: twelve floats each (P1c, P2c, obs1, obs2, info1, info2:
// all of them floats in the reference too, widened when read) and a tag = slot | state << 16 (slots fit 16 bits: n <= 65535).
// state: 1 = both edges active, 2 = removed after the first classification.  Column-major with stride cap, in LDS or in HBM.
struct CorrTable {
    float *f;      // [12][cap]
    uint32_t *tag; // [cap]
    int cap, n;
};
__host__ __device__ constexpr size_t corr_table_bytes(int cap) { return (size_t)cap * (12 * sizeof(float) + sizeof(uint32_t)); }

__device__ __forceinline__ int corr_state(const CorrTable &T, int k) { return (int)(T.tag[k] >> 16); }
__device__ __forceinline__ int corr_slot(const CorrTable &T, int k) { return (int)(T.tag[k] & 0xffffu); }
__device__ __forceinline__ void corr_remove(const CorrTable &T, int k) { T.tag[k] = (T.tag[k] & 0xffffu) | (2u << 16); }
__device__ __forceinline__ void corr_store(const CorrTable &T, int k, const float v[12], int slot)
{
#pragma unroll
    for (int j = 0; j < 12; j++) T.f[j * (size_t)T.cap + k] = v[j];
    T.tag[k] = (uint32_t)slot | (1u << 16);
}
__device__ __forceinline__ void corr_load(const CorrTable &T, int k, double P1[3], double P2[3], double obs1[2], double obs2[2], double &info1, double &info2)
{
    float v[12];
#pragma unroll
    for (int j = 0; j < 12; j++) v[j] = T.f[j * (size_t)T.cap + k];
    P1[0] = (double)v[0]; P1[1] = (double)v[1]; P1[2] = (double)v[2];
    P2[0] = (double)v[3]; P2[1] = (double)v[4]; P2[2] = (double)v[5];
    obs1[0] = (double)v[6]; obs1[1] = (double)v[7]; obs2[0] = (double)v[8]; obs2[1] = (double)v[9];
    info1 = (double)v[10]; info2 = (double)v[11];
}

// One edge's share of the normal equations (BaseBinaryEdge::constructQuadraticForm with a robust kernel, only the Sim3 vertex free):
// b += B^T (rho[1] * -omega e), A += B^T (rho[1] omega) B, and rho[0] into the robust chi2.
__device__ __forceinline__ void sim3_accumulate(const double (&J)[2][7], const double e[2], double info, double delta, double (&acc)[S3_NVAL])
{
    const double chi = e[0] * (info * e[0]) + e[1] * (info * e[1]);
    double rho0, rho1;
    huber(chi, delta, rho0, rho1);
    acc[S3_CHI] += rho0;
    const double wi = info * rho1;
    const double or0 = -(info * e[0]) * rho1, or1 = -(info * e[1]) * rho1;
    int k = 0;
#pragma unroll
    for (int a = 0; a < 7; a++) {
        const double ja0 = J[0][a] * wi, ja1 = J[1][a] * wi;
#pragma unroll
        for (int b = a; b < 7; b++) { acc[k] += ja0 * J[0][b] + ja1 * J[1][b]; k++; }
        acc[28 + a] += J[0][a] * or0 + J[1][a] * or1;
    }
}

// One pass over the active correspondences at `est`: s_tot[0..27] = H (upper), [28..34] = b, [35] = robust chi2 over both edges of
// every active correspondence, [36] = #active correspondences, left in LDS (the 7 x 7 solve reads them from there).  The Jacobian is
// g2o's numeric one: central differences over the pass's 14 perturbed Sim3s, scaled by 1 / (2 * 1e-9).  Three barriers.
//
// The sums: 37 values do not fit the 32 of the transposing row reduction, so it runs twice -- once on 32 values (H and b[0..3], two left
// per lane) and once on 8 (b[4..6], chi2, count; three of its four steps halve the values, the fourth is a plain exchange) -- 38
// exchanges, where widening to 64 values would cost 60 and 24 more accumulator registers.  Then the 16 rows are summed in order.
template <int THREADS>
__device__ void sim3_eval_pass(const CorrTable &T, const Sim3D &est, bool fix_scale, const CamK &c, double delta,
                               double *s_sims /*[15][16]*/, double *s_rows /*[THREADS/16][40]*/, double *s_tot /*[40]*/, double &chi_out, double &cnt_out)
{
    sim3_perturb(est, fix_scale, s_sims);
    double acc[S3_NVAL];
#pragma unroll
    for (int k = 0; k < S3_NVAL; k++) acc[k] = 0.0;
    const double scalar = 1.0 / (2 * 1e-9);
    for (int k = threadIdx.x; k < T.n; k += THREADS) {
        if (corr_state(T, k) != 1) continue;
        double P1[3], P2[3], obs1[2], obs2[2], info1, info2;
        corr_load(T, k, P1, P2, obs1, obs2, info1, info2);
        double J12[2][7], J21[2][7], e12[2], e21[2];
#pragma unroll
        for (int d = 0; d < 7; d++) {
            double ep[2], em[2];
            sim3_edge_error(sim3_load(s_sims + (2 * d) * S3_SIM_STRIDE), c, P2, obs1, ep);
            sim3_edge_error(sim3_load(s_sims + (2 * d + 1) * S3_SIM_STRIDE), c, P2, obs1, em);
            J12[0][d] = scalar * (ep[0] - em[0]); J12[1][d] = scalar * (ep[1] - em[1]);
            sim3_edge_error(sim3_load(s_sims + (2 * d) * S3_SIM_STRIDE + 8), c, P1, obs2, ep);
            sim3_edge_error(sim3_load(s_sims + (2 * d + 1) * S3_SIM_STRIDE + 8), c, P1, obs2, em);
            J21[0][d] = scalar * (ep[0] - em[0]); J21[1][d] = scalar * (ep[1] - em[1]);
        }
        sim3_edge_error(sim3_load(s_sims + 14 * S3_SIM_STRIDE), c, P2, obs1, e12);
        sim3_edge_error(sim3_load(s_sims + 14 * S3_SIM_STRIDE + 8), c, P1, obs2, e21);
        sim3_accumulate(J12, e12, info1, delta, acc);
        sim3_accumulate(J21, e21, info2, delta, acc);
        acc[S3_CNT] += 1.0;
    }
    const int lane16 = threadIdx.x & 15;
    const int b3 = (lane16 >> 3) & 1, b2 = (lane16 >> 2) & 1, b1 = (lane16 >> 1) & 1, b0 = lane16 & 1;
    const int row = threadIdx.x >> 4;
    row_transpose_step<32, 0>(acc, b3 != 0);
    row_transpose_step<16, 1>(acc, b2 != 0);
    row_transpose_step<8, 2>(acc, b1 != 0);
    row_transpose_step<4, 3>(acc, b0 != 0);
#pragma unroll
    for (int k = 0; k < 2; k++) s_rows[row * S3_NVAL + ((((k * 2 + b0) * 2 + b1) * 2 + b2) * 2 + b3)] = acc[k]; // as eval_pass of the pose stage
    double *v = acc + 32;
    row_transpose_step<8, 0>(v, b3 != 0);
    row_transpose_step<4, 1>(v, b2 != 0);
    row_transpose_step<2, 2>(v, b1 != 0);
    v[0] += dpp_f64(v[0], 3); // the partner i ^ 1 holds the same value's other half
    if (!b0) s_rows[row * S3_NVAL + 32 + ((b1 * 2 + b2) * 2 + b3)] = v[0];
    __syncthreads();
    if (threadIdx.x < S3_NVAL) {
        double t = 0.0;
#pragma unroll 8
        for (int r = 0; r < THREADS / 16; r++) t += s_rows[r * S3_NVAL + threadIdx.x];
        s_tot[threadIdx.x] = t;
    }
    __syncthreads();
    chi_out = s_tot[S3_CHI];
    cnt_out = s_tot[S3_CNT];
}

} // namespace
