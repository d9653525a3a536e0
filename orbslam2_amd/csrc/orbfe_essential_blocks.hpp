// orbfe_essential_blocks.hpp -- the device building blocks of orbfe_essential_graph.hip (Optimizer::OptimizeEssentialGraph): g2o's
// Sim3::log, EdgeSim3's error with BaseBinaryEdge's numeric Jacobians, one edge's share of the normal equations, the 7 x 7 pieces of the
// block LDLT, the pose recovery and the point correction; in a header so that a test-only translation unit
// (tests/essential_blocks/essential_blocks.hip) can run each alone against the float64 model (tests/essential_graph_model.py).
// The exponential and oplus are orbfe_sim3_blocks.hpp's (section 4n): there is no second one.  Device code only.
//
// g2o call map:  eg_to_rotation           = Quaterniond::toRotationMatrix (Eigen/src/Geometry/Quaternion.h)
//                eg_log                   = Sim3::log (types/sim3.h:148-230): all four branches, deltaR, skew, W, W.lu().solve(t)
//                eg_lu3_solve             = PartialPivLU<Matrix3d>::solve, pivot and operation order as DESIGN.md section 4s states them
//                eg_mul / _inverse / _map = operator*, inverse, map (:266-272, :233-236, :144-146), restated WITHOUT contraction
//                eg_edge_error            = EdgeSim3::computeError (types/types_seven_dof_expmap.h:106-114): log(C * S_i * S_j.inverse())
//                eg_perturb_one           = one of the 14 oplus calls per vertex of BaseBinaryEdge::linearizeOplus, with its inverse
//                eg_edge_linearize        = computeError + linearizeOplus (core/base_binary_edge.hpp:176-197): e, Ji, Jj
//                eg_solve                 = BlockSolver::solve with LinearSolverEigen: the block LDLT along the plan, one workgroup
//                eg_recover_pose          = :1043-1053: toRotationMatrix, t * (1. / s), Converter::toCvSE3
//                eg_correct_point         = :1076-1084: correctedSwr.map(Srw.map((double)pos)) cast to float
#pragma once
#include "orbfe_sim3_blocks.hpp"

// Everything below is stated operation by operation: host code compiled with -ffp-contract=off gives the same bits wherever no libm
// call (log, acos, sin, cos, sqrt is exact) is involved.  The recovery and the point correction call none.
#pragma clang fp contract(off)

namespace {

constexpr int EG_THREADS = 256;      // the one workgroup of eg_kernel
constexpr int EG_EDGE_DOUBLES = 105; // per edge: e[7], Ji[7][7] (row = error component, column = dof), Jj[7][7]
constexpr int EG_PERT_STRIDE = S3_NSIM * S3_SIM_STRIDE; // per vertex: 14 perturbed Sim3s and the estimate, each with its inverse

__device__ inline void eg_quat_rotate(const Se3 &q, const double v[3], double out[3]) // Quaternion::_transformVector
{
    double uv[3] = {q.y * v[2] - q.z * v[1], q.z * v[0] - q.x * v[2], q.x * v[1] - q.y * v[0]};
    uv[0] += uv[0]; uv[1] += uv[1]; uv[2] += uv[2];
    const double c[3] = {q.y * uv[2] - q.z * uv[1], q.z * uv[0] - q.x * uv[2], q.x * uv[1] - q.y * uv[0]};
#pragma unroll
    for (int i = 0; i < 3; i++) out[i] = (v[i] + q.w * uv[i]) + c[i];
}

__device__ inline void eg_map(const Sim3D &S, const double p[3], double out[3])
{
    double r[3];
    eg_quat_rotate(S.q, p, r);
#pragma unroll
    for (int i = 0; i < 3; i++) out[i] = S.s * r[i] + S.q.t[i];
}

__device__ inline Sim3D eg_mul(const Sim3D &a, const Sim3D &b)
{
    Sim3D r;
    double rt[3];
    eg_quat_rotate(a.q, b.q.t, rt);
#pragma unroll
    for (int i = 0; i < 3; i++) r.q.t[i] = a.s * rt[i] + a.q.t[i];
    r.q.w = ((a.q.w * b.q.w - a.q.x * b.q.x) - a.q.y * b.q.y) - a.q.z * b.q.z;
    r.q.x = ((a.q.w * b.q.x + a.q.x * b.q.w) + a.q.y * b.q.z) - a.q.z * b.q.y;
    r.q.y = ((a.q.w * b.q.y + a.q.y * b.q.w) + a.q.z * b.q.x) - a.q.x * b.q.z;
    r.q.z = ((a.q.w * b.q.z + a.q.z * b.q.w) + a.q.x * b.q.y) - a.q.y * b.q.x;
    r.s = a.s * b.s;
    return r;
}

__device__ inline Sim3D eg_inverse(const Sim3D &a)
{
    Sim3D r;
    r.q.x = -a.q.x; r.q.y = -a.q.y; r.q.z = -a.q.z; r.q.w = a.q.w;
    const double k = -1. / a.s;
    const double v[3] = {k * a.q.t[0], k * a.q.t[1], k * a.q.t[2]};
    eg_quat_rotate(r.q, v, r.q.t);
    r.s = 1. / a.s;
    return r;
}

__device__ inline void eg_to_rotation(const Se3 &q, double R[3][3])
{
    const double tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z;
    const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
    const double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
    const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
    R[0][0] = 1 - (tyy + tzz); R[0][1] = txy - twz;       R[0][2] = txz + twy;
    R[1][0] = txy + twz;       R[1][1] = 1 - (txx + tzz); R[1][2] = tyz - twx;
    R[2][0] = txz - twy;       R[2][1] = tyz + twx;       R[2][2] = 1 - (txx + tyy);
}

// x = W.lu().solve(t).  Column k = 0, 1, 2: the pivot is the FIRST row i >= k with the largest |W[i][k]| (a later row wins only when
// strictly larger); rows k and pivot swap (t with them); W[i][k] /= W[k][k] for i > k (a true division; skipped for a zero pivot, as
// Eigen does); W[i][j] -= W[i][k] * W[k][j] for i, j > k.  Then c = L^-1 P t top down (c[i] -= the sum over ascending j of
// L[i][j] * c[j], summed first) and x = U^-1 c bottom up (x[i] = (c[i] - sum over ascending j > i of U[i][j] * x[j]) / U[i][i]).
__device__ inline void eg_lu3_solve(double W[3][3], const double t[3], double x[3])
{
    double c[3] = {t[0], t[1], t[2]};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        int piv = k;
        double best = fabs(W[k][k]);
#pragma unroll
        for (int i = k + 1; i < 3; i++)
            if (fabs(W[i][k]) > best) { best = fabs(W[i][k]); piv = i; }
        if (piv != k) {
#pragma unroll
            for (int j = 0; j < 3; j++) { const double tmp = W[k][j]; W[k][j] = W[piv][j]; W[piv][j] = tmp; }
            const double tmp = c[k]; c[k] = c[piv]; c[piv] = tmp;
        }
        if (best != 0.0) {
#pragma unroll
            for (int i = k + 1; i < 3; i++) W[i][k] /= W[k][k];
        }
#pragma unroll
        for (int i = k + 1; i < 3; i++)
#pragma unroll
            for (int j = k + 1; j < 3; j++) W[i][j] -= W[i][k] * W[k][j];
    }
    c[1] -= W[1][0] * c[0];
    c[2] -= W[2][0] * c[0] + W[2][1] * c[1];
    x[2] = c[2] / W[2][2];
    x[1] = (c[1] - W[1][2] * x[2]) / W[1][1];
    x[0] = (c[0] - (W[0][1] * x[1] + W[0][2] * x[2])) / W[0][0];
}

__device__ inline void eg_log(const Sim3D &S, double res[7])
{
    const double s = S.s;
    const double sigma = log(s);
    double R[3][3];
    eg_to_rotation(S.q, R);
    const double d = 0.5 * (R[0][0] + R[1][1] + R[2][2] - 1);
    const double dR[3] = {R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]};
    const double eps = 0.00001;
    double A, B, C, k;
    const bool small_theta = d > 1 - eps;
    double theta = 0.0;
    if (small_theta) k = 0.5;
    else {
        theta = acos(d);
        k = theta / (2 * sqrt(1 - d * d));
    }
    const double om[3] = {k * dR[0], k * dR[1], k * dR[2]};
    if (fabs(sigma) < eps) {
        C = 1;
        if (small_theta) { A = 1. / 2.; B = 1. / 6.; }
        else {
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
            const double theta2 = theta * theta;
            const double a = s * sin(theta), b = s * cos(theta);
            const double c = theta2 + sigma * sigma;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    }
    const double O[3][3] = {{0, -om[2], om[1]}, {om[2], 0, -om[0]}, {-om[1], om[0], 0}};
    double W[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double bo = B * O[i][0], b1 = B * O[i][1], b2 = B * O[i][2]; // (B * Omega) * Omega
            const double o2 = (bo * O[0][j] + b1 * O[1][j]) + b2 * O[2][j];
            W[i][j] = (A * O[i][j] + o2) + C * ((i == j) ? 1.0 : 0.0);
        }
    double ups[3];
    eg_lu3_solve(W, S.q.t, ups);
    res[0] = om[0]; res[1] = om[1]; res[2] = om[2];
    res[3] = ups[0]; res[4] = ups[1]; res[5] = ups[2];
    res[6] = sigma;
}

__device__ inline bool eg_sim3_finite(const Sim3D &S)
{
    return isfinite(S.q.x) && isfinite(S.q.y) && isfinite(S.q.z) && isfinite(S.q.w) && isfinite(S.q.t[0]) && isfinite(S.q.t[1]) && isfinite(S.q.t[2]) && isfinite(S.s);
}

// Sim3(Converter::toMatrix3d(Rcw), Converter::toVector3d(tcw), 1.0) of a float Tcw row (:871-873)
__device__ inline Sim3D eg_sim3_from_Tcw(const float *T)
{
    double R[3][3], t[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) R[i][j] = (double)T[4 * i + j];
        t[i] = (double)T[4 * i + 3];
    }
    return sim3_from_rts(R, t, 1.0);
}

__device__ inline void eg_edge_error(const Sim3D &C, const Sim3D &Si, const Sim3D &Sj_inv, double e[7])
{
    eg_log(eg_mul(eg_mul(C, Si), Sj_inv), e);
}

// entry k of a vertex's table: k = 2 d + (0: +1e-9, 1: -1e-9) along dimension d, k = 14 the estimate; S then S.inverse()
__device__ inline void eg_perturb_one(const Sim3D &est, int k, bool fix_scale, double *dst /*[16]*/)
{
    Sim3D S = est;
    if (k < S3_NSIM - 1) {
        const double delta = 1e-9;
        double u[7];
#pragma unroll
        for (int j = 0; j < 7; j++) u[j] = (j == (k >> 1)) ? ((k & 1) ? -delta : delta) : 0.0;
        S = sim3_oplus(u, fix_scale, est);
    }
    sim3_store(S, dst);
    sim3_store(eg_inverse(S), dst + 8);
}

// e, and the 7 x 7 numeric Jacobian of each free end; a fixed end's block is all zero (g2o builds none)
__device__ inline void eg_edge_linearize(const Sim3D &C, const double *pert_i, const double *pert_j, bool free_i, bool free_j, double *out /*[105]*/)
{
    const Sim3D Si = sim3_load(pert_i + 14 * S3_SIM_STRIDE), Sj_inv = sim3_load(pert_j + 14 * S3_SIM_STRIDE + 8);
    double e[7];
    eg_edge_error(C, Si, Sj_inv, e);
#pragma unroll
    for (int k = 0; k < 7; k++) out[k] = e[k];
    const double scalar = 1.0 / (2 * 1e-9);
    for (int d = 0; d < 7; d++) {
        double ep[7], em[7];
        if (free_i) {
            eg_edge_error(C, sim3_load(pert_i + (2 * d) * S3_SIM_STRIDE), Sj_inv, ep);
            eg_edge_error(C, sim3_load(pert_i + (2 * d + 1) * S3_SIM_STRIDE), Sj_inv, em);
        }
#pragma unroll
        for (int k = 0; k < 7; k++) out[7 + 7 * k + d] = free_i ? scalar * (ep[k] - em[k]) : 0.0;
        if (free_j) {
            eg_edge_error(C, Si, sim3_load(pert_j + (2 * d) * S3_SIM_STRIDE + 8), ep);
            eg_edge_error(C, Si, sim3_load(pert_j + (2 * d + 1) * S3_SIM_STRIDE + 8), em);
        }
#pragma unroll
        for (int k = 0; k < 7; k++) out[56 + 7 * k + d] = free_j ? scalar * (ep[k] - em[k]) : 0.0;
    }
}

// element (a, b) of X^T Y for two 7 x 7 Jacobians: the sum over the error components in order
__device__ __forceinline__ double eg_jtj(const double *X, const double *Y, int a, int b)
{
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 7; k++) s += X[7 * k + a] * Y[7 * k + b];
    return s;
}

// Element (a, b) of one slot of H: the slot's edges in the plan's order.  A diagonal slot sums Jx^T Jx of the edge's side; an
// off-diagonal slot Ji^T Jj where the flag is set (the slot's rows are vertex i's), Jj^T Ji otherwise.
__device__ inline double eg_slot_element(const int32_t *slot_edges, int begin, int end, bool diagonal, const double *edge_blocks, int a, int b)
{
    double s = 0.0;
    for (int q = begin; q < end; q++) {
        const int32_t w = slot_edges[q];
        const double *E = edge_blocks + (size_t)(w >> 1) * EG_EDGE_DOUBLES;
        const double *Ji = E + 7, *Jj = E + 56;
        if (diagonal) s += (w & 1) ? eg_jtj(Jj, Jj, a, b) : eg_jtj(Ji, Ji, a, b);
        else s += (w & 1) ? eg_jtj(Ji, Jj, a, b) : eg_jtj(Jj, Ji, a, b);
    }
    return s;
}

// element a of b_p = - sum over the diagonal slot's edges of J^T e
__device__ inline double eg_rhs_element(const int32_t *slot_edges, int begin, int end, const double *edge_blocks, int a)
{
    double s = 0.0;
    for (int q = begin; q < end; q++) {
        const int32_t w = slot_edges[q];
        const double *E = edge_blocks + (size_t)(w >> 1) * EG_EDGE_DOUBLES;
        const double *J = E + ((w & 1) ? 56 : 7);
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 7; k++) t += J[7 * k + a] * E[k];
        s -= t;
    }
    return s;
}

// LDLT without pivoting of one 7 x 7 diagonal block in place (the lower triangle is read; afterwards the strict lower triangle holds
// the unit L and the diagonal D), and z = L^-1 y in place.  False when a pivot is zero or not finite (SimplicialLDLT's failure).
__device__ inline bool eg_ldlt7(double *A /*[49]*/, double *y /*[7]*/)
{
    bool ok = true;
    for (int j = 0; j < 7; j++) {
        double d = A[7 * j + j];
        for (int k = 0; k < j; k++) d -= A[7 * j + k] * A[7 * j + k] * A[7 * k + k];
        A[7 * j + j] = d;
        if (d == 0.0 || !isfinite(d)) ok = false;
        for (int i = j + 1; i < 7; i++) {
            double v = A[7 * i + j];
            for (int k = 0; k < j; k++) v -= A[7 * i + k] * A[7 * j + k] * A[7 * k + k];
            A[7 * i + j] = v / d;
        }
    }
    for (int i = 1; i < 7; i++) {
        double v = y[i];
        for (int k = 0; k < i; k++) v -= A[7 * i + k] * y[k];
        y[i] = v;
    }
    return ok;
}

// row `a` of an off-diagonal block B of the pivot's column becomes row a of X = B L^-T D^-1, in place
__device__ inline void eg_block_row_solve(double *Brow /*[7]*/, const double *Dp /*[49], factored*/)
{
    double v[7];
#pragma unroll
    for (int c = 0; c < 7; c++) {
        double s = Brow[c];
        for (int k = 0; k < c; k++) s -= v[k] * Dp[7 * c + k];
        v[c] = s;
    }
#pragma unroll
    for (int c = 0; c < 7; c++) Brow[c] = v[c] / Dp[7 * c + c];
}

// every lane receives the sum of all lanes' values: the tree's order is fixed
__device__ inline double eg_block_sum(double v, double *s_red)
{
    s_red[threadIdx.x] = v;
    __syncthreads();
    for (int off = EG_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) s_red[threadIdx.x] += s_red[threadIdx.x + off];
        __syncthreads();
    }
    const double r = s_red[0];
    __syncthreads();
    return r;
}

struct EgPlan {
    const int32_t *pos, *colptr, *rowidx, *slot_ptr, *slot_edges, *upd_ptr, *upd;
    int n_free, n_slots;
};

// (H + lambda I) x = b along the plan; x is left in y = F + 49 n_slots, in elimination order.  False: a zero or non-finite pivot.
__device__ inline bool eg_solve(const double *H, const double *b, const EgPlan &P, double lambda, double *F, int *s_fail)
{
    double *y = F + (size_t)P.n_slots * 49;
    for (int t = threadIdx.x; t < P.n_slots * 49; t += EG_THREADS) {
        const int s = t / 49, r = t - s * 49;
        F[t] = H[t] + ((s < P.n_free && r / 7 == r % 7) ? lambda : 0.0);
    }
    for (int t = threadIdx.x; t < P.n_free * 7; t += EG_THREADS) y[t] = b[t];
    if (threadIdx.x == 0) *s_fail = 0;
    __syncthreads();
    for (int p = 0; p < P.n_free; p++) {
        double *Dp = F + (size_t)p * 49;
        if (threadIdx.x == 0 && !eg_ldlt7(Dp, y + 7 * (size_t)p)) *s_fail = 1;
        __syncthreads();
        const int cb = P.colptr[p], m = P.colptr[p + 1] - cb;
        for (int t = threadIdx.x; t < m * 7; t += EG_THREADS) eg_block_row_solve(F + (size_t)(P.n_free + cb + t / 7) * 49 + (t % 7) * 7, Dp);
        __syncthreads();
        const int ub = P.upd_ptr[p], nu = P.upd_ptr[p + 1] - ub;
        for (int t = threadIdx.x; t < nu * 49 + m * 7; t += EG_THREADS) {
            if (t < nu * 49) {
                const int u = t / 49, r = t - u * 49, ra = r / 7, rb = r % 7;
                const int32_t *U = P.upd + 3 * (size_t)(ub + u);
                const double *Xr = F + (size_t)U[0] * 49 + 7 * ra, *Xc = F + (size_t)U[1] * 49 + 7 * rb;
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 7; k++) s += (Xr[k] * Dp[8 * k]) * Xc[k];
                F[(size_t)U[2] * 49 + r] -= s;
            } else {
                const int t2 = t - nu * 49, blk = t2 / 7, ra = t2 % 7;
                const double *X = F + (size_t)(P.n_free + cb + blk) * 49 + 7 * ra;
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 7; k++) s += X[k] * y[7 * (size_t)p + k];
                y[7 * (size_t)P.rowidx[cb + blk] + ra] -= s;
            }
        }
        __syncthreads();
    }
    for (int p = P.n_free - 1; p >= 0; p--) {
        if (threadIdx.x < 64) { // wave 0: lanes 0 .. 6 gather, lane 0 substitutes back
            const double *Dp = F + (size_t)p * 49;
            const int lane = threadIdx.x;
            double acc = 0.0;
            if (lane < 7) {
                acc = y[7 * (size_t)p + lane] / Dp[8 * lane];
                for (int q = P.colptr[p]; q < P.colptr[p + 1]; q++) {
                    const double *X = F + (size_t)(P.n_free + q) * 49, *xr = y + 7 * (size_t)P.rowidx[q];
                    double s = 0.0;
#pragma unroll
                    for (int c = 0; c < 7; c++) s += X[7 * c + lane] * xr[c];
                    acc -= s;
                }
            }
            double xs[7];
#pragma unroll
            for (int i = 6; i >= 0; i--) {
                double v = __shfl(acc, i, 64);
#pragma unroll
                for (int k = i + 1; k < 7; k++) v -= Dp[7 * k + i] * xs[k];
                xs[i] = v;
            }
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < 7; i++) y[7 * (size_t)p + i] = xs[i];
            }
        }
        __syncthreads();
    }
    return *s_fail == 0;
}

// :1043-1053: R = toRotationMatrix(), t * (1. / s), Converter::toCvSE3 (floats); and Ow = -R^T t as orbfe_lba.hip patches it
__device__ inline void eg_recover_pose(const Sim3D &S, float *T /*[16]*/, float *Ow /*[3] or null*/)
{
    double R[3][3];
    eg_to_rotation(S.q, R);
    const double inv = 1. / S.s;
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) T[4 * i + j] = (float)R[i][j];
        T[4 * i + 3] = (float)(S.q.t[i] * inv);
    }
    T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
    if (Ow) {
#pragma unroll
        for (int i = 0; i < 3; i++) {
            double s = 0;
#pragma unroll
            for (int m = 0; m < 3; m++) s += (double)T[4 * m + i] * (double)T[4 * m + 3];
            Ow[i] = (float)(-1.0 * s);
        }
    }
}

__device__ inline void eg_correct_point(const Sim3D &Srw, const Sim3D &correctedSwr, float *pos /*[3]*/)
{
    const double p[3] = {(double)pos[0], (double)pos[1], (double)pos[2]};
    double m[3], o[3];
    eg_map(Srw, p, m);
    eg_map(correctedSwr, m, o);
    pos[0] = (float)o[0]; pos[1] = (float)o[1]; pos[2] = (float)o[2];
}

} // namespace
