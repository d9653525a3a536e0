// orbfe_lba_blocks.hpp -- the device building blocks of orbfe_lba.hip (Optimizer::LocalBundleAdjustment): the two binary edges with
// their analytic Jacobians, the per-edge blocks of the normal equations, Eigen's 3 x 3 inverse, the workgroup's fixed-order sum and the
// dense LDLT without pivoting of the reduced system, then lba_kernel with its phases and the carving of its scratch.  The SE3 algebra is
// orbfe_pose_blocks.hpp's.  Include it from a HIP translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/orbfe.h"
#include "orbfe_arena.hpp"
#include "orbfe_pose_blocks.hpp" // Se3, CamD, se3_*, edge_error, and this stage's fp contract(fast) pragma

#pragma clang fp contract(fast)

namespace {

constexpr int LBA_THREADS = 512;           // one workgroup drives the whole call; 256 VGPRs per lane at two waves per SIMD
constexpr int LBA_WAVES = LBA_THREADS / 64;
constexpr int LBA_LIN = 48;                // doubles per edge of the linearisation: Hpl (18, [6][3]) | Hpp_e (21, upper) | bp_e (6) | 3 unused
constexpr int LBA_W = 24;                  // doubles per edge and trial: Hpl * Dinv (18) | Hpl * (Dinv * b_l) (6)
constexpr int LBA_PT = 9;                  // doubles per point of the linearisation: Hll (6, upper) | b_l (3)

// the reduced system of K free keyframes: (6K + 1) rows of 6K doubles, the right-hand side as the last row
__host__ __device__ constexpr size_t lba_system_bytes(int K) { return sizeof(double) * (size_t)(6 * K + 1) * (size_t)(6 * K); }

// -DORBFE_LBA_TIMING (never shipped; tools/lba_phases.py): cycles of thread 0 per phase, summed over the call
#ifdef ORBFE_LBA_TIMING
__device__ long long g_lba_cycles[8]; // [0] vertices, edges, sort [1] error passes [2] per-point linearisation [3] Hpp walk [4] Dinv and Hpl Dinv [5] Schur rows [6] LDLT [7] landmark step, update, accept
#define LBA_T(var) const long long var = clock64()
#define LBA_ACC(slot, a, b) do { if (threadIdx.x == 0) g_lba_cycles[slot] += (b) - (a); } while (0)
#else
#define LBA_T(var)
#define LBA_ACC(slot, a, b)
#endif

__device__ __forceinline__ int upper6(int i, int j) // index of (i, j), i <= j, in a packed upper triangle of a 6 x 6, row-major
{
    return i * 6 - i * (i - 1) / 2 + (j - i);
}

__device__ inline void quat_matrix(const Se3 &q, double R[3][3]) // Quaterniond::toRotationMatrix
{
    const double tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z;
    const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
    const double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x, tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
    R[0][0] = 1 - (tyy + tzz); R[0][1] = txy - twz; R[0][2] = txz + twy;
    R[1][0] = txy + twz; R[1][1] = 1 - (txx + tzz); R[1][2] = tyz - twx;
    R[2][0] = txz - twy; R[2][1] = tyz + twx; R[2][2] = 1 - (txx + tyy);
}

// RobustKernelHuber::robustify (core/robust_kernel_impl.cpp:78-91): rho[0] returned, rho[1] in w
__device__ __forceinline__ double lba_huber(double chi, double delta, double &w)
{
    const double dsqr = delta * delta;
    w = 1.0;
    if (chi > dsqr) {
        const double sq = sqrt(chi);
        w = delta / sq;
        return 2 * sq * delta - dsqr;
    }
    return chi;
}

// One edge at (pose q, point X): what buildSystem adds for it.  Hll (6, upper) and bl (3) are ACCUMULATED into; lin (LBA_LIN doubles,
// may be null for an edge on a held or fixed keyframe) receives Hpl, the edge's share of Hpp and of b_p.
// linearizeOplus of EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ (types_six_dof_expmap.cpp:103-139, :188-234).
__device__ inline void lba_edge_blocks(const Se3 &q, const CamD &c, const double X[3], const double obs[3], bool stereo, double info, bool robust,
                                       double delta_mono, double delta_stereo, double *Hll, double *bl, double *lin)
{
    double err[3], p[3], invz;
    const double chi = edge_error(q, c, X, obs, stereo, info, err, p, &invz);
    double w = 1.0;
    if (robust) lba_huber(chi, stereo ? delta_stereo : delta_mono, w);
    const double wi = w * info; // robustInformation: rho[1] * _information
    double R[3][3];
    quat_matrix(q, R);
    const double x = p[0], y = p[1], invz_2 = invz * invz;
    double Ji[3][3], Jj[3][6];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        Ji[0][k] = -c.fx * R[0][k] * invz + c.fx * x * R[2][k] * invz_2;
        Ji[1][k] = -c.fy * R[1][k] * invz + c.fy * y * R[2][k] * invz_2;
        Ji[2][k] = stereo ? Ji[0][k] - c.bf * R[2][k] * invz_2 : 0.0;
    }
    Jj[0][0] = x * y * invz_2 * c.fx;
    Jj[0][1] = -(1 + (x * x * invz_2)) * c.fx;
    Jj[0][2] = y * invz * c.fx;
    Jj[0][3] = -invz * c.fx;
    Jj[0][4] = 0;
    Jj[0][5] = x * invz_2 * c.fx;
    Jj[1][0] = (1 + y * y * invz_2) * c.fy;
    Jj[1][1] = -x * y * invz_2 * c.fy;
    Jj[1][2] = -x * invz * c.fy;
    Jj[1][3] = 0;
    Jj[1][4] = -invz * c.fy;
    Jj[1][5] = y * invz_2 * c.fy;
    Jj[2][0] = stereo ? Jj[0][0] - c.bf * y * invz_2 : 0.0;
    Jj[2][1] = stereo ? Jj[0][1] + c.bf * x * invz_2 : 0.0;
    Jj[2][2] = stereo ? Jj[0][2] : 0.0;
    Jj[2][3] = stereo ? Jj[0][3] : 0.0;
    Jj[2][4] = 0.0;
    Jj[2][5] = stereo ? Jj[0][5] - c.bf * invz_2 : 0.0;
    const double we[3] = {wi * err[0], wi * err[1], wi * err[2]};
    double iw[3][3]; // W Ji
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int k = 0; k < 3; k++) iw[r][k] = wi * Ji[r][k];
    {
        int k = 0;
#pragma unroll
        for (int a = 0; a < 3; a++) {
#pragma unroll
            for (int b = a; b < 3; b++) Hll[k++] += Ji[0][a] * iw[0][b] + Ji[1][a] * iw[1][b] + Ji[2][a] * iw[2][b];
            bl[a] -= Ji[0][a] * we[0] + Ji[1][a] * we[1] + Ji[2][a] * we[2];
        }
    }
    if (!lin) return;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) lin[3 * a + b] = Jj[0][a] * iw[0][b] + Jj[1][a] * iw[1][b] + Jj[2][a] * iw[2][b];
    {
        int k = 18;
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int b = a; b < 6; b++) lin[k++] = wi * (Jj[0][a] * Jj[0][b] + Jj[1][a] * Jj[1][b] + Jj[2][a] * Jj[2][b]);
#pragma unroll
        for (int a = 0; a < 6; a++) lin[39 + a] = -(Jj[0][a] * we[0] + Jj[1][a] * we[1] + Jj[2][a] * we[2]);
    }
}

// Eigen's inverse() of a 3 x 3 (Inverse.h, compute_inverse<., 3>): cofactors over the determinant.  D symmetric, given as its upper
// triangle plus lambda on the diagonal; all nine entries of the result are formed as Eigen forms them.
__device__ inline void lba_inverse3(const double *Hu, double lambda, double inv[9])
{
    const double m[3][3] = {{Hu[0] + lambda, Hu[1], Hu[2]}, {Hu[1], Hu[3] + lambda, Hu[4]}, {Hu[2], Hu[4], Hu[5] + lambda}};
    double cof[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            cof[i][j] = m[i1][j1] * m[i2][j2] - m[i1][j2] * m[i2][j1];
        }
    const double det = m[0][0] * cof[0][0] + m[0][1] * cof[0][1] + m[0][2] * cof[0][2];
    const double invdet = 1.0 / det;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) inv[3 * i + j] = cof[j][i] * invdet;
}

// The sum of one value per thread, the same bits in every thread and on every run: a butterfly inside each wave (both partners add
// the same two numbers), then the wave sums in wave order.  Two barriers.
template <int THREADS>
__device__ inline double lba_block_sum(double v, double *s_part /*[THREADS / 64]*/)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; w++) t += s_part[w];
    __syncthreads();
    return t;
}

// Dense LDLT without pivoting of the n x n system whose lower triangle is S[i * n + j] (j <= i) and whose right-hand side is row n
// (S[n * n + j]); every thread of the workgroup calls it.  SimplicialLDLT's failure rule: an exactly zero pivot ends the factorisation
// and the call returns false (a NaN pivot does not).  On success row n holds x.  The right-hand side rides along as one more row of L,
// which is the forward substitution and the division by D; the transposed solve follows.  n == 0 succeeds.
template <int THREADS>
__device__ inline bool lba_ldlt_solve(double *S, int n)
{
    for (int k = 0; k < n; k++) {
        const double d = S[(size_t)k * n + k];
        if (d == 0.0) return false; // the same value in every thread
        for (int i = k + 1 + threadIdx.x; i <= n; i += THREADS) S[(size_t)i * n + k] /= d;
        __syncthreads();
        const long long rows = n - k, cols = n - k - 1; // rows k + 1 .. n, columns k + 1 .. n - 1; their product passes int32 from n = 46,341 on
        for (long long idx = threadIdx.x; idx < rows * cols; idx += THREADS) {
            const int i = k + 1 + (int)(idx / cols), j = k + 1 + (int)(idx % cols);
            if (j <= i) S[(size_t)i * n + j] -= S[(size_t)i * n + k] * (d * S[(size_t)j * n + k]);
        }
        __syncthreads();
    }
    double *x = S + (size_t)n * n;
    for (int k = n - 1; k > 0; k--) {
        const double xk = x[k];
        for (int j = threadIdx.x; j < k; j += THREADS) x[j] -= S[(size_t)k * n + j] * xk;
        __syncthreads();
    }
    return true;
}

// ---------------------------------------------------------------------------------------------------------------- the kernel
// lba_kernel and its phases (the call map is at the head of orbfe_lba.hip, which keeps the entry points).  Here so that the test-only
// translation unit can run one linearisation and Schur reduction alone.
constexpr size_t LBA_LDS_REQUEST = 128 * 1024; // of the CU's 160 KiB
static_assert(lba_system_bytes(ORBFE_LBA_LDS_KEYFRAMES) <= LBA_LDS_REQUEST, "the reduced system of ORBFE_LBA_LDS_KEYFRAMES free keyframes fits the LDS the kernel requests");
static_assert(lba_system_bytes(ORBFE_LBA_LDS_KEYFRAMES + 1) > LBA_LDS_REQUEST, "and one keyframe more does not: the constant is derived, not chosen");

enum : uint8_t { EF_VALID = 1, EF_STEREO = 2, EF_LEVEL1 = 4 };
enum : uint8_t { PF_OK = 1, PF_ACTIVE = 2 };

struct LbaArgs {
    // the call's arrays
    const orbfe_ba_keyframe *kfs;
    const uint8_t *role;
    float *Tcw;
    const int32_t *row, *obs_off, *obs_kf, *obs_idx;
    float *pos;
    orbfe_obs_keyframe *obs_kfs;
    uint8_t *edge_code;
    double *edge_chi2;
    int32_t *erase, *n_erase, *status;
    orbfe_lba_info *info;
    int32_t n_kfs, max_free, n_pts, n_rows, n_obs, nlevels;
    // scratch
    int32_t *e_kf, *e_pt, *sorted, *cnt /*[LBA_THREADS][max_free]*/, *kf_free /*[n_kfs]*/, *f_kf, *f_start /*[max_free + 1]*/, *f_red;
    float *e_obs;      // [n_obs][4]: x, y, u_right, information
    int32_t *e_red;    // [n_obs], per round: the reduced index of the edge's keyframe when the edge is at level 0 on an active free keyframe, else -1
    uint8_t *e_flag, *p_flag;
    double *chi_a, *chi_b, *chi_f, *e_lin, *e_w;
    double *pose_e, *pose_t; // [n_kfs][8]
    double *f_H /*[max_free][27]*/, *f_x /*[max_free][6]*/;
    double *X_e, *X_t, *p_lin /*[n_pts][9]*/, *p_dinv /*[n_pts][9]*/, *p_xl /*[n_pts][3]*/;
    double *system; // the HBM variant's reduced system
    float inv_sigma2[ORBFE_MAX_LEVELS];
    float fx, fy, cx, cy, bf;
    double delta_mono, delta_stereo;
};

struct LbaShared {
    double part[LBA_WAVES];
    unsigned long long max_bits;
    int wave_cnt[LBA_WAVES];
    int invalid, n_free, n_red, counts[4], n_erase;
};

__device__ __forceinline__ Se3 load_pose(const double *p) { Se3 q; q.x = p[0]; q.y = p[1]; q.z = p[2]; q.w = p[3]; q.t[0] = p[4]; q.t[1] = p[5]; q.t[2] = p[6]; return q; }
__device__ __forceinline__ void store_pose(double *p, const Se3 &q) { p[0] = q.x; p[1] = q.y; p[2] = q.z; p[3] = q.w; p[4] = q.t[0]; p[5] = q.t[1]; p[6] = q.t[2]; }

__device__ __forceinline__ void load_edge(const LbaArgs &a, int j, double obs[3], double &info, bool stereo)
{
    const float4 o = *(const float4 *)(a.e_obs + 4 * (size_t)j);
    obs[0] = (double)o.x; obs[1] = (double)o.y; obs[2] = stereo ? (double)o.z : 0.0; info = (double)o.w;
}

// computeActiveErrors + activeRobustChi2 at (pose, X): chi2 of every level-0 edge into chi_out, the robust total returned
__device__ double lba_errors(const LbaArgs &a, LbaShared &sh, const CamD &cam, const double *pose, const double *X, bool robust, double *chi_out)
{
    LBA_T(t0);
    double acc = 0.0;
    for (int j = threadIdx.x; j < a.n_obs; j += LBA_THREADS) {
        const uint8_t f = a.e_flag[j];
        if ((f & (EF_VALID | EF_LEVEL1)) != EF_VALID) continue;
        const bool stereo = (f & EF_STEREO) != 0;
        double obs[3], info, err[3], p[3];
        load_edge(a, j, obs, info, stereo);
        const Se3 q = load_pose(pose + 8 * (size_t)a.e_kf[j]);
        const double *Xq = X + 3 * (size_t)a.e_pt[j];
        const double Xw[3] = {Xq[0], Xq[1], Xq[2]};
        const double chi = edge_error(q, cam, Xw, obs, stereo, info, err, p);
        chi_out[j] = chi;
        double w;
        acc += robust ? lba_huber(chi, stereo ? a.delta_stereo : a.delta_mono, w) : chi;
    }
    const double total = lba_block_sum<LBA_THREADS>(acc, sh.part);
    LBA_T(t1);
    LBA_ACC(1, t0, t1);
    return total;
}

// buildSystem at the accepted estimate; with want_max the largest |diagonal entry| of the active blocks is returned (computeLambdaInit)
__device__ double lba_linearize(const LbaArgs &a, LbaShared &sh, const CamD &cam, bool robust, bool want_max)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    LBA_T(t0);
    if (threadIdx.x == 0) sh.max_bits = 0ull;
    __syncthreads();
    double mx = 0.0;
    for (int q = threadIdx.x; q < a.n_pts; q += LBA_THREADS) {
        if (!(a.p_flag[q] & PF_ACTIVE)) continue;
        const double X[3] = {a.X_e[3 * (size_t)q], a.X_e[3 * (size_t)q + 1], a.X_e[3 * (size_t)q + 2]};
        double H[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
        const int j1 = a.obs_off[q + 1];
        for (int j = a.obs_off[q]; j < j1; j++) {
            const uint8_t f = a.e_flag[j];
            if ((f & (EF_VALID | EF_LEVEL1)) != EF_VALID) continue;
            const bool stereo = (f & EF_STEREO) != 0;
            double obs[3], info;
            load_edge(a, j, obs, info, stereo);
            const int k = a.e_kf[j];
            const int fr = a.kf_free[k];
            const bool on_free = fr >= 0 && a.f_red[fr] >= 0;
            lba_edge_blocks(load_pose(a.pose_e + 8 * (size_t)k), cam, X, obs, stereo, info, robust, a.delta_mono, a.delta_stereo, H, b,
                            on_free ? a.e_lin + LBA_LIN * (size_t)j : nullptr);
        }
        double *pl = a.p_lin + LBA_PT * (size_t)q;
#pragma unroll
        for (int i = 0; i < 6; i++) pl[i] = H[i];
#pragma unroll
        for (int i = 0; i < 3; i++) pl[6 + i] = b[i];
        const double dg[3] = {fabs(H[0]), fabs(H[3]), fabs(H[5])};
#pragma unroll
        for (int i = 0; i < 3; i++) if (dg[i] == dg[i]) mx = fmax(mx, dg[i]);
    }
    __syncthreads(); // the per-edge blocks are in place
    LBA_T(t1);
    LBA_ACC(2, t0, t1);
    // Hpp and b_p of every active free keyframe: its wave walks its edges in edge order, lane l sums value l
    for (int fr = wave; fr < sh.n_free; fr += LBA_WAVES) {
        if (a.f_red[fr] < 0) continue;
        double acc = 0.0;
        const int e1 = a.f_start[fr + 1];
        for (int e0 = a.f_start[fr]; e0 < e1; e0 += 64) { // 64 edges' indices at once, one per lane; then edge by edge in edge order
            int mine = -1;
            if (e0 + lane < e1) { mine = a.sorted[e0 + lane]; if (a.e_red[mine] < 0) mine = -1; }
            unsigned long long todo = __ballot(mine >= 0);
            while (todo) {
                const int l = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const int j = __shfl(mine, l, 64);
                if (lane < 27) acc += a.e_lin[LBA_LIN * (size_t)j + 18 + lane];
            }
        }
        if (lane < 27) a.f_H[27 * (size_t)fr + lane] = acc;
        const bool diag = lane == 0 || lane == 6 || lane == 11 || lane == 15 || lane == 18 || lane == 20;
        if (diag && acc == acc) mx = fmax(mx, fabs(acc));
    }
    if (want_max) atomicMax(&sh.max_bits, (unsigned long long)__double_as_longlong(mx)); // non-negative doubles order as their bits: an integer maximum, no order dependence
    __syncthreads();
    LBA_T(t2);
    LBA_ACC(3, t1, t2);
    return __longlong_as_double((long long)sh.max_bits);
}

// setLambda + BlockSolver::solve.  Returns false on a zero pivot of the reduced system (x then keeps what it held).
template <bool IN_LDS>
__device__ bool lba_solve(const LbaArgs &a, LbaShared &sh, double *S, double lambda, bool reduce_only = false)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = 6 * sh.n_red;
    LBA_T(t0);
    // Dinv = (Hll + lambda I)^-1 per point, and per edge on a free keyframe Hpl Dinv and Hpl (Dinv b_l)
    for (int q = threadIdx.x; q < a.n_pts; q += LBA_THREADS) {
        if (!(a.p_flag[q] & PF_ACTIVE)) continue;
        const double *pl = a.p_lin + LBA_PT * (size_t)q;
        double Hu[6], inv[9];
#pragma unroll
        for (int i = 0; i < 6; i++) Hu[i] = pl[i];
        lba_inverse3(Hu, lambda, inv);
        double *pd = a.p_dinv + 9 * (size_t)q;
#pragma unroll
        for (int i = 0; i < 9; i++) pd[i] = inv[i];
        double db[3];
#pragma unroll
        for (int i = 0; i < 3; i++) db[i] = inv[3 * i] * pl[6] + inv[3 * i + 1] * pl[7] + inv[3 * i + 2] * pl[8];
        const int j1 = a.obs_off[q + 1];
        for (int j = a.obs_off[q]; j < j1; j++) {
            if ((a.e_flag[j] & (EF_VALID | EF_LEVEL1)) != EF_VALID) continue;
            const int fr = a.kf_free[a.e_kf[j]];
            if (fr < 0 || a.f_red[fr] < 0) continue;
            const double *B = a.e_lin + LBA_LIN * (size_t)j;
            double *W = a.e_w + LBA_W * (size_t)j;
#pragma unroll
            for (int r = 0; r < 6; r++) {
#pragma unroll
                for (int c = 0; c < 3; c++) W[3 * r + c] = B[3 * r] * inv[c] + B[3 * r + 1] * inv[3 + c] + B[3 * r + 2] * inv[6 + c];
                W[18 + r] = B[3 * r] * db[0] + B[3 * r + 1] * db[1] + B[3 * r + 2] * db[2];
            }
        }
    }
    for (size_t i = threadIdx.x; i < (size_t)(n + 1) * n; i += LBA_THREADS) S[i] = 0.0;
    __syncthreads();
    LBA_T(t1);
    LBA_ACC(4, t0, t1);
    // Block row r1 of Hschur = Hpp + lambda I - sum_p Hpl Dinv Hpl^T, blocks (r1, r2 >= r1), stored at the transposed (lower) position;
    // lane 6 r + c owns entry (r, c) of every block of the row, lanes 36 .. 41 the row's share of bschur.
    for (int fr = wave; fr < sh.n_free; fr += LBA_WAVES) {
        const int r1 = a.f_red[fr];
        if (r1 < 0) continue;
        const int r = lane < 36 ? lane / 6 : lane - 36, c = lane < 36 ? lane % 6 : 0;
        if (lane < 36) {
            const double h = a.f_H[27 * (size_t)fr + upper6(r < c ? r : c, r < c ? c : r)];
            S[(size_t)(6 * r1 + c) * n + 6 * r1 + r] = h + (r == c ? lambda : 0.0);
        }
        double bacc = 0.0;
        const int e1 = a.f_start[fr + 1];
        // The indices travel in batches -- 64 of the keyframe's edges with their points' list bounds, then 64 entries of a point's list,
        // one per lane -- and are handed round by shuffles; the sums still run edge by edge and partner by partner in list order.
        for (int e0 = a.f_start[fr]; e0 < e1; e0 += 64) {
            int mine = -1, mine_g0 = 0, mine_g1 = 0;
            if (e0 + lane < e1) {
                mine = a.sorted[e0 + lane];
                if (a.e_red[mine] < 0) mine = -1;
                else { const int q = a.e_pt[mine]; mine_g0 = a.obs_off[q]; mine_g1 = a.obs_off[q + 1]; }
            }
            unsigned long long todo = __ballot(mine >= 0);
            while (todo) {
                const int l = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const int j = __shfl(mine, l, 64), g0 = __shfl(mine_g0, l, 64), g1 = __shfl(mine_g1, l, 64);
                const double *W = a.e_w + LBA_W * (size_t)j;
                if (lane >= 36 && lane < 42) bacc += W[18 + r];
                double w0 = 0, w1 = 0, w2 = 0;
                if (lane < 36) { w0 = W[3 * r]; w1 = W[3 * r + 1]; w2 = W[3 * r + 2]; }
                for (int gb = g0; gb < g1; gb += 64) { // the point's list, in order: the partner blocks (r2 >= r1 leaves out the inactive, -1)
                    const int red = gb + lane < g1 ? a.e_red[gb + lane] : -1;
                    unsigned long long partners = __ballot(red >= r1);
                    while (partners) {
                        const int pl = __ffsll((long long)partners) - 1;
                        partners &= partners - 1;
                        const int r2 = __shfl(red, pl, 64);
                        if (lane < 36) {
                            const double *B = a.e_lin + LBA_LIN * (size_t)(gb + pl);
                            S[(size_t)(6 * r2 + c) * n + 6 * r1 + r] -= w0 * B[3 * c] + w1 * B[3 * c + 1] + w2 * B[3 * c + 2];
                        }
                    }
                }
            }
        }
        if (lane >= 36 && lane < 42) S[(size_t)n * n + 6 * r1 + r] = a.f_H[27 * (size_t)fr + 21 + r] - bacc;
    }
    __syncthreads();
    LBA_T(t2);
    LBA_ACC(5, t1, t2);
    if (reduce_only) return true; // the reduced system as it goes into the factorisation (tests/lba_blocks)
    const bool solved = lba_ldlt_solve<LBA_THREADS>(S, n);
    LBA_T(t3);
    LBA_ACC(6, t2, t3);
    if (!solved) return false;
    for (int i = threadIdx.x; i < n; i += LBA_THREADS) a.f_x[i] = S[(size_t)n * n + i]; // indexed by position in the reduced system
    __syncthreads();
    // the landmark step (:459-481): xl = Dinv (b_l - sum Hpl^T xp)
    for (int q = threadIdx.x; q < a.n_pts; q += LBA_THREADS) {
        if (!(a.p_flag[q] & PF_ACTIVE)) continue;
        const double *pl = a.p_lin + LBA_PT * (size_t)q;
        double cl[3] = {pl[6], pl[7], pl[8]};
        const int j1 = a.obs_off[q + 1];
        for (int j = a.obs_off[q]; j < j1; j++) {
            if ((a.e_flag[j] & (EF_VALID | EF_LEVEL1)) != EF_VALID) continue;
            const int fr = a.kf_free[a.e_kf[j]];
            if (fr < 0 || a.f_red[fr] < 0) continue;
            const double *B = a.e_lin + LBA_LIN * (size_t)j;
            const double *xp = a.f_x + 6 * (size_t)a.f_red[fr];
#pragma unroll
            for (int r = 0; r < 6; r++) {
                cl[0] -= B[3 * r] * xp[r]; cl[1] -= B[3 * r + 1] * xp[r]; cl[2] -= B[3 * r + 2] * xp[r];
            }
        }
        const double *inv = a.p_dinv + 9 * (size_t)q;
#pragma unroll
        for (int i = 0; i < 3; i++) a.p_xl[3 * (size_t)q + i] = inv[3 * i] * cl[0] + inv[3 * i + 1] * cl[1] + inv[3 * i + 2] * cl[2];
    }
    __syncthreads();
    LBA_T(t4);
    LBA_ACC(7, t3, t4);
    return true;
}

// computeScale over both parts of the update, then the update itself into the trial estimates
__device__ double lba_apply(const LbaArgs &a, LbaShared &sh, double lambda)
{
    LBA_T(t0);
    double acc = 0.0;
    for (int fr = threadIdx.x; fr < sh.n_free; fr += LBA_THREADS) {
        const int r1 = a.f_red[fr];
        if (r1 < 0) continue;
        const double *xp = a.f_x + 6 * (size_t)r1, *bp = a.f_H + 27 * (size_t)fr + 21;
        double u[6];
#pragma unroll
        for (int i = 0; i < 6; i++) { u[i] = xp[i]; acc += u[i] * (lambda * u[i] + bp[i]); }
        const int k = a.f_kf[fr];
        store_pose(a.pose_t + 8 * (size_t)k, se3_mul(se3_exp(u), load_pose(a.pose_e + 8 * (size_t)k)));
    }
    for (int q = threadIdx.x; q < a.n_pts; q += LBA_THREADS) {
        if (!(a.p_flag[q] & PF_ACTIVE)) continue;
        const double *pl = a.p_lin + LBA_PT * (size_t)q;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const double x = a.p_xl[3 * (size_t)q + i];
            acc += x * (lambda * x + pl[6 + i]);
            a.X_t[3 * (size_t)q + i] = a.X_e[3 * (size_t)q + i] + x;
        }
    }
    const double scale = lba_block_sum<LBA_THREADS>(acc, sh.part) + 1e-3; // ends in a barrier: the trial estimates are in place
    LBA_T(t1);
    LBA_ACC(7, t0, t1);
    return scale;
}

__device__ void lba_accept(const LbaArgs &a, LbaShared &sh)
{
    for (int fr = threadIdx.x; fr < sh.n_free; fr += LBA_THREADS) {
        if (a.f_red[fr] < 0) continue;
        const int k = a.f_kf[fr];
        for (int i = 0; i < 7; i++) a.pose_e[8 * (size_t)k + i] = a.pose_t[8 * (size_t)k + i];
    }
    for (int q = threadIdx.x; q < a.n_pts; q += LBA_THREADS) {
        if (!(a.p_flag[q] & PF_ACTIVE)) continue;
        for (int i = 0; i < 3; i++) a.X_e[3 * (size_t)q + i] = a.X_t[3 * (size_t)q + i];
    }
    __syncthreads();
}

struct LbaRound { int iterations, trials; double chi_start, chi_end, lambda; bool ran; };

// initializeOptimization(0) + optimize(iterations): the level-0 edges, the vertices they touch
template <bool IN_LDS>
__device__ LbaRound lba_optimize(const LbaArgs &a, LbaShared &sh, double *S, const CamD &cam, int iterations, bool robust, bool stop_after_reduction = false)
{
    LbaRound R = {0, 0, 0.0, 0.0, 0.0, false};
    // the active set: a vertex without a level-0 edge takes no part (it keeps its estimate and gives the reduced system no block)
    for (int fr = threadIdx.x; fr < sh.n_free; fr += LBA_THREADS) a.f_red[fr] = -1;
    if (threadIdx.x == 0) { sh.counts[0] = 0; sh.counts[1] = 0; }
    __syncthreads();
    int n_act = 0, n_pts_act = 0;
    for (int q = threadIdx.x; q < a.n_pts; q += LBA_THREADS) {
        uint8_t pf = a.p_flag[q] & PF_OK;
        if (pf) {
            int cnt = 0;
            const int j1 = a.obs_off[q + 1];
            for (int j = a.obs_off[q]; j < j1; j++) {
                if ((a.e_flag[j] & (EF_VALID | EF_LEVEL1)) != EF_VALID) continue;
                cnt++;
                const int fr = a.kf_free[a.e_kf[j]];
                if (fr >= 0) a.f_red[fr] = 0; // every writer writes this value
            }
            if (cnt) { pf |= PF_ACTIVE; n_pts_act++; }
            n_act += cnt;
        }
        a.p_flag[q] = pf;
    }
    if (n_act) atomicAdd(&sh.counts[0], n_act); // integer counts: the order does not matter
    if (n_pts_act) atomicAdd(&sh.counts[1], n_pts_act);
    __syncthreads();
    if (threadIdx.x == 0) {
        int r = 0;
        for (int fr = 0; fr < sh.n_free; fr++) if (a.f_red[fr] == 0) a.f_red[fr] = r++;
        sh.n_red = r;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < a.n_obs; j += LBA_THREADS) { // what the keyframe walks test per edge: one load instead of four dependent ones
        int red = -1;
        if ((a.e_flag[j] & (EF_VALID | EF_LEVEL1)) == EF_VALID) { const int fr = a.kf_free[a.e_kf[j]]; if (fr >= 0) red = a.f_red[fr]; }
        a.e_red[j] = red;
    }
    __syncthreads();
    if (sh.counts[0] == 0) return R; // optimize() returns before doing anything
    R.ran = true;
    // the trial estimates of the vertices that take no part are the estimates
    for (int i = threadIdx.x; i < 8 * a.n_kfs; i += LBA_THREADS) a.pose_t[i] = a.pose_e[i];
    for (size_t i = threadIdx.x; i < 3 * (size_t)a.n_pts; i += LBA_THREADS) a.X_t[i] = a.X_e[i];
    for (int i = threadIdx.x; i < 6 * sh.n_red; i += LBA_THREADS) a.f_x[i] = 0.0;
    for (size_t i = threadIdx.x; i < 3 * (size_t)a.n_pts; i += LBA_THREADS) a.p_xl[i] = 0.0;
    __syncthreads();
    double *chi_est = a.chi_a, *chi_trial = a.chi_b, *chi_last;
    double current_chi = lba_errors(a, sh, cam, a.pose_e, a.X_e, robust, chi_est);
    chi_last = chi_est;
    R.chi_start = current_chi;
    const double max_diag = lba_linearize(a, sh, cam, robust, true);
    double lambda = 1e-5 * max_diag, ni = 2.0;
    int lm_bad = 0;
    if (stop_after_reduction) { // test-only instances: the first linearisation and its Schur reduction, left in p_lin and S
        lba_solve<IN_LDS>(a, sh, S, lambda, true);
        R.lambda = lambda;
        return R;
    }
    for (int it = 0; it < iterations; it++) {
        R.iterations++;
        chi_last = chi_est; // computeActiveErrors at the current estimate
        const double ini_chi = current_chi;
        double rho = 0.0;
        int qmax = 0;
        do {
            const bool ok2 = lba_solve<IN_LDS>(a, sh, S, lambda);
            const double scale = lba_apply(a, sh, lambda);
            const double chi_s = lba_errors(a, sh, cam, a.pose_t, a.X_t, robust, chi_trial);
            chi_last = chi_trial;
            const double temp_chi = ok2 ? chi_s : DBL_MAX;
            rho = (current_chi - temp_chi) / scale;
            if (rho > 0 && isfinite(temp_chi)) {
                const double r21 = 2 * rho - 1;
                double alpha = 1.0 - r21 * r21 * r21;
                alpha = fmin(alpha, 2.0 / 3.0);
                lambda *= fmax(1.0 / 3.0, alpha);
                ni = 2;
                current_chi = temp_chi;
                lba_accept(a, sh);
                double *t = chi_est; chi_est = chi_trial; chi_trial = t;
                chi_last = chi_est;
                lba_linearize(a, sh, cam, robust, false);
            } else {
                lambda *= ni;
                ni *= 2;
            }
            qmax++;
        } while (rho < 0 && qmax < 10);
        R.trials += qmax;
        if (qmax == 10 || rho == 0) break;
        if ((ini_chi - current_chi) * 1e3 < ini_chi) lm_bad++;
        else lm_bad = 0;
        if (lm_bad >= 3) break;
    }
    // BaseEdge::chi2() of the edges this round evaluated: the last evaluation, accepted or not
    for (int j = threadIdx.x; j < a.n_obs; j += LBA_THREADS)
        if ((a.e_flag[j] & (EF_VALID | EF_LEVEL1)) == EF_VALID) a.chi_f[j] = chi_last[j];
    __syncthreads();
    R.chi_end = current_chi;
    R.lambda = lambda;
    return R;
}

// chi2() > 5.991 / 7.815 || !isDepthPositive(): chi2 as the last evaluation left it, the depth at the CURRENT estimates
__device__ void lba_classify(const LbaArgs &a, uint8_t bit)
{
    for (int j = threadIdx.x; j < a.n_obs; j += LBA_THREADS) {
        const uint8_t f = a.e_flag[j];
        if (!(f & EF_VALID)) continue;
        const Se3 q = load_pose(a.pose_e + 8 * (size_t)a.e_kf[j]);
        const double *Xq = a.X_e + 3 * (size_t)a.e_pt[j];
        const double Xw[3] = {Xq[0], Xq[1], Xq[2]};
        double p[3];
        se3_map(q, Xw, p);
        const bool bad = a.chi_f[j] > ((f & EF_STEREO) ? 7.815 : 5.991) || !(p[2] > 0.0);
        if (bad) {
            a.edge_code[j] |= bit;
            if (bit == 1) a.e_flag[j] = f | EF_LEVEL1;
        }
    }
    __syncthreads();
}

// vToErase in the reference's order: every flagged mono edge in edge order, then every flagged stereo edge
__device__ void lba_erase_list(const LbaArgs &a, LbaShared &sh)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int n_out = 0;
    for (int pass = 0; pass < 2; pass++) {
        for (int j0 = 0; j0 < a.n_obs; j0 += LBA_THREADS) {
            const int j = j0 + threadIdx.x;
            bool hit = false;
            if (j < a.n_obs) {
                const uint8_t f = a.e_flag[j];
                hit = (f & EF_VALID) && (a.edge_code[j] & 2) && (((f & EF_STEREO) != 0) == (pass == 1));
            }
            const unsigned long long vote = __ballot(hit);
            if (lane == 0) sh.wave_cnt[wave] = __popcll(vote);
            __syncthreads();
            int before = n_out, total = 0;
#pragma unroll
            for (int w = 0; w < LBA_WAVES; w++) {
                const int cw = sh.wave_cnt[w];
                if (w < wave) before += cw;
                total += cw;
            }
            if (hit) {
                const int k = before + __popcll(vote & ((1ull << lane) - 1)); // < number of valid edges <= n_obs
                a.erase[2 * (size_t)k] = a.e_kf[j];
                a.erase[2 * (size_t)k + 1] = a.e_pt[j];
            }
            n_out += total;
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) *a.n_erase = n_out;
}

// STOP_AFTER_REDUCTION: the test-only instances of tests/lba_blocks, which end after round 1's first linearisation and Schur reduction
// and leave the reduced system in a.system (copied there from the LDS), lambda in info->lambda_last, the system's keyframes in info->n_free
template <bool IN_LDS, bool STOP_AFTER_REDUCTION = false>
__global__ __launch_bounds__(LBA_THREADS) void lba_kernel(const LbaArgs a)
{
    extern __shared__ double s_dyn[];
    __shared__ LbaShared sh;
    double *S = IN_LDS ? s_dyn : a.system;
    LBA_T(t_begin);
    const CamD cam = {(double)a.fx, (double)a.fy, (double)a.cx, (double)a.cy, (double)a.bf};
    if (threadIdx.x == 0) { sh.invalid = 0; sh.n_free = 0; sh.n_red = 0; sh.counts[0] = sh.counts[1] = sh.counts[2] = sh.counts[3] = 0; }
    __syncthreads();

    // ---- vertices of the keyframes (:566-590); the free ones are numbered in keyframe order
    for (int k = threadIdx.x; k < a.n_kfs; k += LBA_THREADS) {
        const int r = a.role[k];
        if (r > ORBFE_BA_FIXED) sh.invalid = 1; // every writer writes this value
        if (r >= ORBFE_BA_LOCAL && r <= ORBFE_BA_FIXED) store_pose(a.pose_e + 8 * (size_t)k, se3_from_cv(a.Tcw + 16 * (size_t)k));
        a.kf_free[k] = -1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int nf = 0;
        for (int k = 0; k < a.n_kfs; k++)
            if (a.role[k] == ORBFE_BA_LOCAL) {
                if (nf < a.max_free) { a.kf_free[k] = nf; a.f_kf[nf] = k; }
                nf++;
            }
        sh.n_free = nf;
    }
    __syncthreads();
    if (sh.n_free > a.max_free) { // more free keyframes than the host sized the variant for: nothing else is written
        if (threadIdx.x == 0) *a.status = ORBFE_ERR_CAPACITY;
        return;
    }

    // ---- point vertices and edges (:616-697), each index checked before it becomes an address
    for (int j = threadIdx.x; j < a.n_obs; j += LBA_THREADS) { a.e_flag[j] = 0; a.edge_code[j] = 0; a.chi_f[j] = 0.0; a.e_pt[j] = 0; a.e_kf[j] = 0; }
    __syncthreads();
    int n_mono = 0, n_stereo = 0;
    for (int q = threadIdx.x; q < a.n_pts; q += LBA_THREADS) {
        a.p_flag[q] = 0;
        const int j0 = a.obs_off[q], j1 = a.obs_off[q + 1];
        if (j0 < 0 || j1 < j0 || j1 > a.n_obs) { sh.invalid = 1; continue; }
        const int row = a.row ? a.row[q] : q;
        if (row < 0 || row >= a.n_rows) {
            sh.invalid = 1;
            for (int j = j0; j < j1; j++) a.edge_code[j] = 8;
            continue;
        }
        a.p_flag[q] = PF_OK;
#pragma unroll
        for (int i = 0; i < 3; i++) a.X_e[3 * (size_t)q + i] = (double)a.pos[3 * (size_t)row + i];
        for (int j = j0; j < j1; j++) {
            const int k = a.obs_kf[j], i = a.obs_idx[j];
            uint8_t code = 0, flag = 0;
            if (k < 0 || k >= a.n_kfs) code = 8;
            else {
                const int r = a.role[k];
                if (r > ORBFE_BA_FIXED) code = 8;
                else if (r == ORBFE_BA_SKIP) code = 4;
                else {
                    const orbfe_ba_keyframe kf = a.kfs[k];
                    if (i < 0 || i >= kf.n || !kf.keys_un || !kf.u_right) code = 8;
                    else {
                        const KeyPointPOD kp = ((const KeyPointPOD *)kf.keys_un)[i];
                        if (kp.octave < 0 || kp.octave >= a.nlevels) code = 8;
                        else {
                            const float ur = kf.u_right[i];
                            const bool stereo = !(ur < 0);
                            flag = EF_VALID | (stereo ? EF_STEREO : 0);
                            *(float4 *)(a.e_obs + 4 * (size_t)j) = make_float4(kp.x, kp.y, ur, a.inv_sigma2[kp.octave]);
                            a.e_kf[j] = k;
                            a.e_pt[j] = q;
                            if (stereo) n_stereo++; else n_mono++;
                        }
                    }
                }
            }
            if (code == 8) sh.invalid = 1;
            a.edge_code[j] = code;
            a.e_flag[j] = flag;
        }
    }
    if (n_mono) atomicAdd(&sh.counts[2], n_mono);
    if (n_stereo) atomicAdd(&sh.counts[3], n_stereo);
    __syncthreads();
    const int total_mono = sh.counts[2], total_stereo = sh.counts[3];
    if (total_mono + total_stereo == 0) { // no edge at all: status, counts of zero and the codes
        if (threadIdx.x == 0) {
            orbfe_lba_info z = {};
            *a.info = z;
            *a.n_erase = 0;
            *a.status = sh.invalid ? ORBFE_ERR_INVALID : 0;
        }
        if (a.edge_chi2) for (int j = threadIdx.x; j < a.n_obs; j += LBA_THREADS) a.edge_chi2[j] = 0.0;
        return;
    }

    // ---- the edges of every free keyframe in edge order: a counting sort, thread t owning the t-th chunk of the edge array
    {
        const int nf = sh.n_free;
        const int chunk = (a.n_obs + LBA_THREADS - 1) / LBA_THREADS;
        const int c0 = min((long long)a.n_obs, (long long)chunk * threadIdx.x), c1 = min((long long)a.n_obs, (long long)chunk * (threadIdx.x + 1));
        int32_t *mine = a.cnt + (size_t)threadIdx.x * nf;
        for (int f = 0; f < nf; f++) mine[f] = 0;
        for (int j = c0; j < c1; j++)
            if (a.e_flag[j] & EF_VALID) { const int fr = a.kf_free[a.e_kf[j]]; if (fr >= 0) mine[fr]++; }
        __syncthreads();
        for (int f = threadIdx.x; f < nf; f += LBA_THREADS) {
            int run = 0;
            for (int t = 0; t < LBA_THREADS; t++) { const int v = a.cnt[(size_t)t * nf + f]; a.cnt[(size_t)t * nf + f] = run; run += v; }
            a.f_red[f] = run; // the keyframe's edge count, until the scan below
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int run = 0;
            for (int f = 0; f < nf; f++) { a.f_start[f] = run; run += a.f_red[f]; }
            a.f_start[nf] = run;
        }
        __syncthreads();
        for (int j = c0; j < c1; j++)
            if (a.e_flag[j] & EF_VALID) { const int fr = a.kf_free[a.e_kf[j]]; if (fr >= 0) a.sorted[a.f_start[fr] + mine[fr]++] = j; }
        __syncthreads();
    }

    LBA_T(t_setup);
    LBA_ACC(0, t_begin, t_setup);
    // ---- optimize(5) with Huber, the first test, optimize(10) without the kernel, the second test (:703-787)
    if constexpr (STOP_AFTER_REDUCTION) {
        const LbaRound r0 = lba_optimize<IN_LDS>(a, sh, S, cam, 5, true, true);
        const size_t cells = (size_t)(6 * sh.n_red + 1) * (size_t)(6 * sh.n_red);
        if (IN_LDS) for (size_t i = threadIdx.x; i < cells; i += LBA_THREADS) a.system[i] = S[i];
        if (threadIdx.x == 0) {
            orbfe_lba_info o = {};
            o.n_free = sh.n_red; o.n_points = sh.counts[1]; o.lambda_last = r0.lambda; o.chi2_start = r0.chi_start;
            *a.info = o;
            *a.status = sh.invalid ? ORBFE_ERR_INVALID : 0;
        }
        return;
    }
    const LbaRound r1 = lba_optimize<IN_LDS>(a, sh, S, cam, 5, true);
    const int n_free_active = sh.n_red, n_points_active = sh.counts[1];
    __syncthreads();
    lba_classify(a, 1);
    const LbaRound r2 = lba_optimize<IN_LDS>(a, sh, S, cam, 10, false);
    lba_classify(a, 2);
    lba_erase_list(a, sh);

    // ---- recover (:806-821): SetPose of every local keyframe with its Ow, SetWorldPos of every point
    for (int k = threadIdx.x; k < a.n_kfs; k += LBA_THREADS) {
        const int r = a.role[k];
        if (r != ORBFE_BA_LOCAL && r != ORBFE_BA_LOCAL_HELD) continue;
        float T[16];
        se3_to_cv(load_pose(a.pose_e + 8 * (size_t)k), T);
#pragma unroll
        for (int i = 0; i < 16; i++) a.Tcw[16 * (size_t)k + i] = T[i];
        if (a.obs_kfs) {
#pragma unroll
            for (int i = 0; i < 3; i++) { // Ow = -Rwc * tcw: one gemm with alpha -1, a double sum over k rounded once
                double s = 0;
#pragma unroll
                for (int m = 0; m < 3; m++) s += (double)T[4 * m + i] * (double)T[4 * m + 3];
                a.obs_kfs[k].Ow[i] = (float)(-1.0 * s);
            }
        }
    }
    for (int q = threadIdx.x; q < a.n_pts; q += LBA_THREADS) {
        if (!(a.p_flag[q] & PF_OK)) continue;
        const int row = a.row ? a.row[q] : q;
#pragma unroll
        for (int i = 0; i < 3; i++) a.pos[3 * (size_t)row + i] = (float)a.X_e[3 * (size_t)q + i];
    }
    if (a.edge_chi2) for (int j = threadIdx.x; j < a.n_obs; j += LBA_THREADS) a.edge_chi2[j] = a.chi_f[j];
    if (threadIdx.x == 0) {
        orbfe_lba_info o = {};
        o.n_mono = total_mono; o.n_stereo = total_stereo; o.n_free = n_free_active; o.n_points = n_points_active;
        o.iterations[0] = r1.iterations; o.iterations[1] = r2.iterations; o.trials[0] = r1.trials; o.trials[1] = r2.trials;
        o.chi2_start = r1.chi_start; o.chi2_first = r1.chi_end; o.chi2_second = r2.chi_end; o.lambda_last = r2.ran ? r2.lambda : r1.lambda;
        *a.info = o;
        *a.status = sh.invalid ? ORBFE_ERR_INVALID : 0;
    }
}

// The scratch of one call, carved from one buffer: sets the scratch pointers of `a` (whose counts are set) from `base` and returns the
// bytes needed; base == nullptr only sizes.  with_system: room for the reduced system of a.max_free keyframes in HBM.
inline size_t lba_carve(LbaArgs &a, uint8_t *b, bool with_system)
{
    const size_t E = (size_t)a.n_obs, N = (size_t)a.n_pts, K = (size_t)a.n_kfs, F = (size_t)a.max_free;
    orbfe::Arena c(b, 256, 8);
    a.e_lin = c.take<double>(LBA_LIN * E); a.e_w = c.take<double>(LBA_W * E); a.chi_a = c.take<double>(E); a.chi_b = c.take<double>(E); a.chi_f = c.take<double>(E);
    a.pose_e = c.take<double>(8 * K); a.pose_t = c.take<double>(8 * K); a.f_H = c.take<double>(27 * F); a.f_x = c.take<double>(6 * F); a.X_e = c.take<double>(3 * N);
    a.X_t = c.take<double>(3 * N); a.p_lin = c.take<double>(LBA_PT * N); a.p_dinv = c.take<double>(9 * N); a.p_xl = c.take<double>(3 * N);
    a.system = c.take<double>(with_system ? lba_system_bytes(a.max_free) / sizeof(double) : 0); a.e_obs = c.take<float>(4 * E); a.e_kf = c.take<int32_t>(E);
    a.e_pt = c.take<int32_t>(E); a.sorted = c.take<int32_t>(E); a.cnt = c.take<int32_t>(LBA_THREADS * F); a.kf_free = c.take<int32_t>(K); a.f_kf = c.take<int32_t>(F);
    a.f_start = c.take<int32_t>(F + 1); a.f_red = c.take<int32_t>(F); a.e_red = c.take<int32_t>(E); a.e_flag = c.take<uint8_t>(E); a.p_flag = c.take<uint8_t>(N);
    return c.bytes();
}

} // namespace
