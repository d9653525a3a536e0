// orbfe_sim3_ransac.hip -- Sim3Solver (src/Sim3Solver.cc) of LoopClosing::ComputeSim3 (src/LoopClosing.cc:298-378) for every candidate
// keyframe in one asynchronous call.  A hypothesis of Sim3Solver::iterate depends on its three draws only, and iterate returns exactly at
// the hypotheses whose inlier count is > min_inliers and >= every earlier count, so all hypotheses of all candidates are evaluated at
// once and the round-robin of :322-378 becomes a host walk over the fetched events (orbslam2_amd/host/Sim3Solver.h).
//
// Three launches whatever n_cands is; launch boundaries are the only hand-off between workgroups:
//   sim3_filter_kernel   one workgroup per candidate: the constructor's filter (:63-110), survivors compacted in pair order into d_corr
//                        and into the correspondence table (12 floats per row, SoA, in the context's scratch), N and the iteration count
//   sim3_hyp_kernel      grid (chunks of SR_HPW hypotheses, candidates), one wave each: lane h solves hypothesis h of the chunk in
//                        registers (draws, ComputeSim3 :227-338), then the wave walks the correspondences 64 at a time for each
//                        hypothesis of the chunk (CheckInliers :341-365); one 64-bit ballot per step is two words of the bit row and, by
//                        popcount, the count.  The table is staged in the LDS up to ORBFE_SIM3_RANSAC_LDS_SLOTS and read from HBM above.
//   sim3_events_kernel   one wave per candidate: the prefix maximum of the counts and the events in ascending order
// No atomics, plain vector stores, fixed orders everywhere: bit-reproducible run to run.  The arithmetic is DESIGN.md section 4o; this
// file is compiled without FMA contraction (the Makefile's -ffp-contract=off), every operation below is rounded once.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "orbfe_device.h"
#include "orbfe_host.h"
#include "orbfe_cvmat.hpp"

static_assert(sizeof(orbfe_sim3_ransac_candidate) == 64 && sizeof(orbfe_sim3_hypothesis) == 64, "record sizes are part of the ABI");

namespace {

constexpr int SR_THREADS = 256; // filter and select
constexpr int SR_HPW = 16;      // hypotheses per wave of sim3_hyp_kernel
constexpr int SR_FIELDS = 12;   // X3Dc1[3] X3Dc2[3] P1im1[2] P2im2[2] gate1 gate2
constexpr int SR_HYP_FLOATS = 24; // sR12[9] t12[3] sR21[9] t21[3]

struct RansacArgs {
    const KeyPointPOD *keys1;
    const float *pos1;
    const int32_t *valid1;
    const orbfe_sim3_ransac_candidate *cands;
    const int32_t *its_for_n;
    int32_t *n_corr, *n_its, *corr, *sets;
    orbfe_sim3_hypothesis *hyp;
    uint32_t *bits;
    int32_t *events, *n_events, *status;
    float *table; // [n_cands][SR_FIELDS][cap]
    float T1w[12], gate[ORBFE_MAX_LEVELS];
    float fx, fy, cx, cy;
    int32_t n1, nlevels, max_pairs, max_kf_n, cap, words, fix_scale, min_inliers, max_its;
};

// FromCameraToImage / the tail of Project (:398-402, :418-422): float operations as written
__device__ __forceinline__ void to_image(const float (&X)[3], float fx, float fy, float cx, float cy, float &u, float &v)
{
    const float invz = 1.f / X[2];
    const float x = X[0] * invz, y = X[1] * invz;
    u = fx * x + cx;
    v = fy * y + cy;
}

__global__ __launch_bounds__(SR_THREADS) void sim3_filter_kernel(const RansacArgs a)
{
    __shared__ int s_wave[SR_THREADS / 64];
    __shared__ int s_invalid;
    const int c = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const orbfe_sim3_ransac_candidate rec = a.cands[c];
    if (threadIdx.x == 0) s_invalid = 0;
    bool rec_ok = rec.n >= 0 && rec.n <= a.max_kf_n && rec.keys_un && rec.pos && rec.valid && rec.T2w && rec.pairs && rec.n_pairs && rec.draws;
    int np = rec_ok ? *rec.n_pairs : 0;
    if (np < 0 || np > a.max_pairs) { rec_ok = false; np = 0; }
    float T1w[12], T2w[12];
#pragma unroll
    for (int k = 0; k < 12; k++) { T1w[k] = a.T1w[k]; T2w[k] = rec_ok ? rec.T2w[k] : 0.f; }
    const KeyPointPOD *keys2 = (const KeyPointPOD *)rec.keys_un;
    float *tab = a.table + (size_t)c * SR_FIELDS * a.cap;
    int32_t *corr = a.corr + (size_t)c * 2 * a.max_pairs;
    __syncthreads();
    int n_corr = 0;
    for (int p0 = 0; p0 < np; p0 += SR_THREADS) {
        const int p = p0 + threadIdx.x;
        bool keep = false;
        int i1 = 0, i2 = 0, o1 = 0, o2 = 0;
        if (p < np) {
            i1 = rec.pairs[2 * (size_t)p]; i2 = rec.pairs[2 * (size_t)p + 1];
            bool ok = i1 >= 0 && i1 < a.n1 && i2 >= 0 && i2 < rec.n; // checked before either becomes an address
            if (ok) {
                o1 = a.keys1[i1].octave; o2 = keys2[i2].octave;
                ok = o1 >= 0 && o1 < a.nlevels && o2 >= 0 && o2 < a.nlevels;
            }
            if (!ok) s_invalid = 1; // every lane that writes writes this value
            else keep = a.valid1[i1] != 0 && rec.valid[i2] != 0;
        }
        const u64 vote = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(vote);
        __syncthreads();
        int before = n_corr, total = 0;
#pragma unroll
        for (int w = 0; w < SR_THREADS / 64; w++) {
            const int cw = s_wave[w];
            if (w < wave) before += cw;
            total += cw;
        }
        if (keep) {
            const int j = before + __popcll(vote & ((1ull << lane) - 1)); // < survivors so far <= p < max_pairs <= cap
            const float Xw1[3] = {a.pos1[3 * (size_t)i1], a.pos1[3 * (size_t)i1 + 1], a.pos1[3 * (size_t)i1 + 2]};
            const float Xw2[3] = {rec.pos[3 * (size_t)i2], rec.pos[3 * (size_t)i2 + 1], rec.pos[3 * (size_t)i2 + 2]};
            // Rcw * Xw + tcw: a float cv::Mat product with its `+ C` form (:96, :99)
            const float X1[3] = {row_dot_plus<0>(T1w, Xw1), row_dot_plus<1>(T1w, Xw1), row_dot_plus<2>(T1w, Xw1)};
            const float X2[3] = {row_dot_plus<0>(T2w, Xw2), row_dot_plus<1>(T2w, Xw2), row_dot_plus<2>(T2w, Xw2)};
            float u1, v1, u2, v2;
            to_image(X1, a.fx, a.fy, a.cx, a.cy, u1, v1);
            to_image(X2, a.fx, a.fy, a.cx, a.cy, u2, v2);
            const float row[SR_FIELDS] = {X1[0], X1[1], X1[2], X2[0], X2[1], X2[2], u1, v1, u2, v2, a.gate[o1], a.gate[o2]};
#pragma unroll
            for (int f = 0; f < SR_FIELDS; f++) tab[(size_t)f * a.cap + j] = row[f];
            corr[2 * (size_t)j] = i1; corr[2 * (size_t)j + 1] = i2;
        }
        n_corr += total;
        __syncthreads(); // s_wave is rewritten by the next chunk; after the last one s_invalid is final
    }
    for (int j = n_corr + threadIdx.x; j < a.max_pairs; j += SR_THREADS) { corr[2 * (size_t)j] = -1; corr[2 * (size_t)j + 1] = -1; }
    if (threadIdx.x == 0) {
        int its = a.its_for_n[n_corr]; // n_corr <= np <= max_pairs
        its = n_corr < 3 ? 0 : min(max(its, 0), a.max_its); // three distinct draws need three correspondences
        a.n_corr[c] = n_corr;
        a.n_its[c] = its;
        a.status[c] = (!rec_ok || s_invalid) ? ORBFE_ERR_INVALID : 0;
    }
}

// one rotation of the cyclic two-sided Jacobi on the symmetric A (both triangles kept), V's columns the eigenvectors
template <int P, int Q> __device__ __forceinline__ bool jacobi_rotate(double (&A)[4][4], double (&V)[4][4])
{
    const double apq = A[P][Q], g = fabs(apq);
    if (fabs(A[P][P]) + g == fabs(A[P][P]) && fabs(A[Q][Q]) + g == fabs(A[Q][Q])) { // the skip rule
        A[P][Q] = 0.0; A[Q][P] = 0.0;
        return false;
    }
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
    if (theta < 0) t = -t;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    A[P][P] = A[P][P] - t * apq;
    A[Q][Q] = A[Q][Q] + t * apq;
    A[P][Q] = 0.0; A[Q][P] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; r++)
        if (r != P && r != Q) {
            const double arp = A[r][P], arq = A[r][Q];
            const double np = c * arp - s * arq, nq = s * arp + c * arq;
            A[r][P] = np; A[P][r] = np;
            A[r][Q] = nq; A[Q][r] = nq;
        }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const double vrp = V[r][P], vrq = V[r][Q];
        V[r][P] = c * vrp - s * vrq;
        V[r][Q] = s * vrp + c * vrq;
    }
    return true;
}

// ComputeCentroid (:216-225): cv::reduce(SUM) is a float sum in index order, `/ P.cols` a scale by (float)(1.0 / 3)
__device__ __forceinline__ void centroid(const float (&P)[9], float (&Pr)[9], float (&C)[3])
{
    const float third = (float)(1.0 / 3);
#pragma unroll
    for (int r = 0; r < 3; r++) {
        C[r] = reduce_sum3(P[3 * r], P[3 * r + 1], P[3 * r + 2]) * third;
#pragma unroll
        for (int i = 0; i < 3; i++) Pr[3 * r + i] = P[3 * r + i] - C[r];
    }
}

// ComputeSim3 (:227-338) on the drawn points (column i of P1 / P2 the i-th): R, t, s and h = sR12 t12 sR21 t21
__device__ __forceinline__ void compute_sim3(const float (&P1)[9], const float (&P2)[9], bool fix_scale, float (&R)[9], float (&t)[3], float &s,
                                             float (&h)[SR_HYP_FLOATS])
{
    float Pr1[9], Pr2[9], O1[3], O2[3], Pr1t[9], M[9];
    centroid(P1, Pr1, O1);
    centroid(P2, Pr2, O2);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) Pr1t[3 * r + c] = Pr1[3 * c + r];
    mul3(Pr2, Pr1t, M);
    const float N11 = (M[0] + M[4]) + M[8], N12 = M[5] - M[7], N13 = M[6] - M[2], N14 = M[1] - M[3], N22 = (M[0] - M[4]) - M[8], N23 = M[1] + M[3],
                N24 = M[6] + M[2], N33 = (-M[0] + M[4]) - M[8], N34 = M[5] + M[7], N44 = (-M[0] - M[4]) + M[8];
    double A[4][4] = {{N11, N12, N13, N14}, {N12, N22, N23, N24}, {N13, N23, N33, N34}, {N14, N24, N34, N44}};
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for (int sweep = 0; sweep < 30; sweep++) {
        bool rotated = jacobi_rotate<0, 1>(A, V);
        rotated |= jacobi_rotate<0, 2>(A, V);
        rotated |= jacobi_rotate<0, 3>(A, V);
        rotated |= jacobi_rotate<1, 2>(A, V);
        rotated |= jacobi_rotate<1, 3>(A, V);
        rotated |= jacobi_rotate<2, 3>(A, V);
        if (!rotated) break;
    }
    double top = A[0][0], w = V[0][0], x = V[1][0], y = V[2][0], z = V[3][0];
#pragma unroll
    for (int i = 1; i < 4; i++)
        if (A[i][i] > top) { top = A[i][i]; w = V[0][i]; x = V[1][i]; y = V[2][i]; z = V[3][i]; } // first strict maximum
    // the rotation matrix of the quaternion (w, x, y, z) / |.|; a zero vector part gives I where atan2 + Rodrigues divide 0 / 0
    const double ww = w * w, xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    const double n = ((ww + xx) + yy) + zz;
    R[0] = (float)((((ww + xx) - yy) - zz) / n); R[1] = (float)((2.0 * (xy - wz)) / n); R[2] = (float)((2.0 * (xz + wy)) / n);
    R[3] = (float)((2.0 * (xy + wz)) / n); R[4] = (float)((((ww - xx) + yy) - zz) / n); R[5] = (float)((2.0 * (yz - wx)) / n);
    R[6] = (float)((2.0 * (xz - wy)) / n); R[7] = (float)((2.0 * (yz + wx)) / n); R[8] = (float)((((ww - xx) - yy) + zz) / n);
    float P3[9];
    mul3(R, Pr2, P3);
    if (!fix_scale) {
        const double nom = dot9(Pr1, P3);                 // Mat::dot: a double sum
        const double den = sum_of_squared_floats9(P3);    // cv::pow(., 2) is a float product; den a double sum of them
        s = ratio(nom, den);
    } else
        s = 1.0f;
    // mt12i = O1 - ms12i * mR12i * O2: one gemm, alpha = -s, C = O1
#pragma unroll
    for (int r = 0; r < 3; r++) {
        double sum = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) sum += (double)R[3 * r + k] * (double)O2[k];
        t[r] = (float)(-(double)s * sum + (double)O1[r]);
    }
    const float inv = (float)(1.0 / (double)s); // (1.0 / ms12i) * mR12i.t(): a scale by (float)(1.0 / s)
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            h[3 * r + c] = s * R[3 * r + c];
            h[12 + 3 * r + c] = R[3 * c + r] * inv;
        }
#pragma unroll
    for (int r = 0; r < 3; r++) {
        h[9 + r] = t[r];
        double sum = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) sum += (double)h[12 + 3 * r + k] * (double)t[k];
        h[21 + r] = (float)(-1.0 * sum); // tinv = -sRinv * mt12i: alpha = -1
    }
}

// |a - Project(X)|^2 with Project = [A | b] then the camera (:383-404): the product has its `+ C` form, dist.dot(dist) is a double sum
__device__ __forceinline__ float reproj_error(const float (&X)[3], const float *A, const float *b, float fx, float fy, float cx, float cy, float au, float av)
{
    float P[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        double sum = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) sum += (double)A[3 * r + k] * (double)X[k];
        P[r] = (float)(sum + (double)b[r]);
    }
    float u, v;
    to_image(P, fx, fy, cx, cy, u, v);
    const float d0 = au - u, d1 = av - v;
    return (float)((double)d0 * (double)d0 + (double)d1 * (double)d1);
}

template <bool IN_LDS>
__global__ __launch_bounds__(64) void sim3_hyp_kernel(const RansacArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float s_dyn[]; // [SR_HPW][SR_HYP_FLOATS], then the table when IN_LDS
    float *s_hyp = s_dyn;
    const int c = blockIdx.y, k0 = blockIdx.x * SR_HPW, lane = threadIdx.x;
    const int N = a.n_corr[c], n_its = a.n_its[c]; // written by sim3_filter_kernel: 0 <= N <= max_pairs <= cap
    const float *tab = a.table + (size_t)c * SR_FIELDS * a.cap;
    if constexpr (IN_LDS) {
        float *s_tab = s_dyn + SR_HPW * SR_HYP_FLOATS;
        if (k0 < n_its)
            for (int f = 0; f < SR_FIELDS; f++)
                for (int j = lane; j < N; j += 64) s_tab[f * a.cap + j] = tab[(size_t)f * a.cap + j];
        tab = s_tab;
        __syncthreads();
    }
    orbfe_sim3_hypothesis *hyp = a.hyp + (size_t)c * a.max_its;
    uint32_t *bits = a.bits + (size_t)c * a.max_its * a.words;
    const int k = k0 + lane;
    float R[9], t[3], s = 0.f;
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = 0.f;
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = 0.f;
    if (lane < SR_HPW && k < a.max_its) {
        int ids[3] = {-1, -1, -1};
        if (k < n_its) {
            // DUtils::Random::RandomInt on the raw values, then vAvailableIndices' swap-with-back-and-pop (:164-178): only the drawn
            // positions ever differ from the identity
            const uint32_t *dr = a.cands[c].draws + 3 * (size_t)k;
            const int r0 = (int)(((double)dr[0] / 2147483648.0) * N);
            const int r1 = (int)(((double)dr[1] / 2147483648.0) * (N - 1));
            const int r2 = (int)(((double)dr[2] / 2147483648.0) * (N - 2));
            const int back = r0 == N - 2 ? N - 1 : N - 2; // what position N - 2 holds after the first draw: it moves to position r1
            ids[0] = min(r0, N - 1); // a raw value above RAND_MAX cannot index beyond the table
            ids[1] = r1 == r0 ? N - 1 : min(r1, N - 1);
            ids[2] = r2 == r1 ? back : (r2 == r0 ? N - 1 : min(r2, N - 1));
            float P1[9], P2[9];
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int r = 0; r < 3; r++) {
                    P1[3 * r + i] = tab[(size_t)r * a.cap + ids[i]];
                    P2[3 * r + i] = tab[(size_t)(3 + r) * a.cap + ids[i]];
                }
            float h[SR_HYP_FLOATS];
            compute_sim3(P1, P2, a.fix_scale != 0, R, t, s, h);
#pragma unroll
            for (int i = 0; i < SR_HYP_FLOATS; i++) s_hyp[lane * SR_HYP_FLOATS + i] = h[i];
        }
        if (a.sets) {
            int32_t *sets = a.sets + ((size_t)c * a.max_its + k) * 3;
            sets[0] = ids[0]; sets[1] = ids[1]; sets[2] = ids[2];
        }
    }
    __syncthreads();
    int my_count = 0;
    const int steps = (a.words + 1) >> 1;
    for (int hq = 0; hq < SR_HPW; hq++) {
        const int kq = k0 + hq; // wave-uniform
        if (kq >= a.max_its) break;
        uint32_t *row = bits + (size_t)kq * a.words;
        if (kq >= n_its) {
            for (int w = lane; w < a.words; w += 64) row[w] = 0u;
            continue;
        }
        float T[SR_HYP_FLOATS];
#pragma unroll
        for (int i = 0; i < SR_HYP_FLOATS; i++) T[i] = s_hyp[hq * SR_HYP_FLOATS + i];
        int count = 0;
        for (int st = 0; st < steps; st++) {
            const int j = st * 64 + lane;
            bool inl = false;
            if (j < N) {
                const float X1[3] = {tab[j], tab[(size_t)a.cap + j], tab[(size_t)2 * a.cap + j]};
                const float X2[3] = {tab[(size_t)3 * a.cap + j], tab[(size_t)4 * a.cap + j], tab[(size_t)5 * a.cap + j]};
                const float err1 = reproj_error(X2, T, T + 9, a.fx, a.fy, a.cx, a.cy, tab[(size_t)6 * a.cap + j], tab[(size_t)7 * a.cap + j]);
                const float err2 = reproj_error(X1, T + 12, T + 21, a.fx, a.fy, a.cx, a.cy, tab[(size_t)8 * a.cap + j], tab[(size_t)9 * a.cap + j]);
                inl = err1 < tab[(size_t)10 * a.cap + j] && err2 < tab[(size_t)11 * a.cap + j]; // a NaN error fails `<`
            }
            const u64 vote = __ballot(inl);
            count += __popcll(vote);
            if (lane < 2 && 2 * st + lane < a.words) row[2 * st + lane] = (uint32_t)(vote >> (32 * lane));
        }
        if (lane == hq) my_count = count;
    }
    if (lane < SR_HPW && k < a.max_its) { // the record: 64 bytes, zero from n_its on
        uint32_t rec[16];
        rec[0] = (uint32_t)my_count;
        rec[1] = __float_as_uint(one_nan(s));
#pragma unroll
        for (int i = 0; i < 9; i++) rec[2 + i] = __float_as_uint(one_nan(R[i]));
#pragma unroll
        for (int i = 0; i < 3; i++) rec[11 + i] = __float_as_uint(one_nan(t[i]));
        rec[14] = 0u; rec[15] = 0u;
        uint32_t *out = (uint32_t *)(hyp + k); // the caller's array need only be 4-byte aligned
#pragma unroll
        for (int q = 0; q < 16; q++) out[q] = rec[q];
    }
}

__global__ __launch_bounds__(64) void sim3_events_kernel(const RansacArgs a)
{
    const int c = blockIdx.x, lane = threadIdx.x;
    const int n_its = a.n_its[c];
    const orbfe_sim3_hypothesis *hyp = a.hyp + (size_t)c * a.max_its;
    int32_t *events = a.events + (size_t)c * a.max_its;
    int best = 0, nev = 0; // mnBestInliers starts at 0
    for (int k0 = 0; k0 < n_its; k0 += 64) {
        const int k = k0 + lane;
        const int n = k < n_its ? hyp[k].n_inliers : -1;
        int m = n; // inclusive prefix maximum over the wave
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(m, off, 64);
            if (lane >= off) m = max(m, o);
        }
        int prev = __shfl_up(m, 1, 64);
        prev = lane == 0 ? best : max(prev, best);
        const bool ev = k < n_its && n > a.min_inliers && n >= prev;
        const u64 vote = __ballot(ev);
        if (ev) events[nev + __popcll(vote & ((1ull << lane) - 1))] = k; // < number of iterations so far <= max_its
        nev += __popcll(vote);
        best = max(best, __shfl(m, 63, 64));
    }
    for (int e = nev + lane; e < a.max_its; e += 64) events[e] = -1;
    if (lane == 0) a.n_events[c] = nev;
}

struct SelectArgs {
    const orbfe_sim3_ransac_candidate *cands;
    const int32_t *valid1, *n_corr, *n_its, *corr;
    const uint32_t *bits;
    int32_t *prior12, *valid1_round, *valid2_round, *status;
    int32_t c, k, n1, max_pairs, max_kf_n, max_its, words;
};

__global__ __launch_bounds__(SR_THREADS) void sim3_select_kernel(const SelectArgs a)
{
    __shared__ int s_invalid;
    const orbfe_sim3_ransac_candidate rec = a.cands[a.c];
    const bool rec_ok = rec.n >= 0 && rec.n <= a.max_kf_n && (rec.n == 0 || rec.valid);
    const int n2 = rec_ok ? rec.n : 0;
    const int N = min(max(a.n_corr[a.c], 0), a.max_pairs);
    const bool k_ok = a.k < a.n_its[a.c];
    if (threadIdx.x == 0) s_invalid = (!rec_ok || !k_ok) ? 1 : 0;
    for (int i = threadIdx.x; i < a.n1; i += SR_THREADS) a.prior12[i] = -1;
    for (int i = threadIdx.x; i < n2; i += SR_THREADS) a.valid2_round[i] = rec.valid[i] != 0;
    __syncthreads();
    if (rec_ok && k_ok) {
        const uint32_t *row = a.bits + ((size_t)a.c * a.max_its + a.k) * a.words;
        const int32_t *corr = a.corr + (size_t)a.c * 2 * a.max_pairs;
        for (int j = threadIdx.x; j < N; j += SR_THREADS)
            if ((row[j >> 5] >> (j & 31)) & 1u) {
                const int i1 = corr[2 * (size_t)j], i2 = corr[2 * (size_t)j + 1];
                if (i1 < 0 || i1 >= a.n1 || i2 < 0 || i2 >= n2) { s_invalid = 1; continue; } // checked before either becomes an address
                a.prior12[i1] = i2;       // idx1 is strictly ascending: one writer per slot
                a.valid2_round[i2] = 0;   // every lane that writes writes this value
            }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < a.n1; i += SR_THREADS) a.valid1_round[i] = a.valid1[i] != 0 && a.prior12[i] < 0;
    if (threadIdx.x == 0) *a.status = s_invalid ? ORBFE_ERR_INVALID : 0;
}

size_t hyp_lds_bytes(int cap) { return sizeof(float) * ((size_t)SR_HPW * SR_HYP_FLOATS + (size_t)SR_FIELDS * cap); }

} // namespace

extern "C" int orbfe_enqueue_sim3_ransac_batch(orbfe_context *ctx, const orbfe_grid_keyframe *kf1, const float *T1w, const float *d_pos1,
                                               const int32_t *d_valid1, const orbfe_sim3_ransac_candidate *d_cands, int n_cands, int max_pairs,
                                               int max_kf_n, int fix_scale, int min_inliers, int max_its, const int32_t *d_its_for_n, int32_t *d_n_corr,
                                               int32_t *d_n_its, int32_t *d_corr, int32_t *d_sets, orbfe_sim3_hypothesis *d_hyp, uint32_t *d_inlier_bits,
                                               int32_t *d_events, int32_t *d_n_events, int32_t *d_status, void *stream)
try {
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    ORBFE_ENTRY(ctx);
    if (!kf1 || !T1w || !d_n_corr || !d_n_its || !d_corr || !d_hyp || !d_inlier_bits || !d_events || !d_n_events || !d_status)
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null argument");
    if (n_cands < 0 || n_cands > 65535) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "n_cands = %d (0 .. 65535)", n_cands);
    if (max_pairs < 1 || max_pairs > 65535 || max_kf_n < 0 || max_kf_n > 65535) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "max_pairs = %d (1 .. 65535), max_kf_n = %d (0 .. 65535)", max_pairs, max_kf_n);
    const int n1 = kf1->n;
    if (n1 < 0 || n1 > 65535 || n1 > max_kf_n) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "keyframe 1 with %d keypoints (0 .. max_kf_n = %d)", n1, max_kf_n);
    if (n1 > 0 && (!kf1->keys_un || !d_pos1 || !d_valid1)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null array of keyframe 1");
    if (min_inliers < 3) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "min_inliers = %d: a hypothesis draws three correspondences", min_inliers);
    if (max_its < 1 || max_its > 65536) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "max_its = %d (1 .. 65536)", max_its);
    if (n_cands > 0 && (!d_cands || !d_its_for_n)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null candidate array or iteration table");
    const orbfe_params *cp = &ctx->params;
    if (cp->nlevels < 1 || cp->nlevels > ORBFE_MAX_LEVELS) return orbfe_fail(ctx, ORBFE_ERR_UNSUPPORTED, "nlevels = %d", cp->nlevels);
    if (n_cands == 0) return ORBFE_OK;
    hipStream_t s;
    if (const int rc = orbfe_enqueue_on(ctx, stream, false, &s)) return rc;
    RansacArgs a;
    a.keys1 = (const KeyPointPOD *)kf1->keys_un; a.pos1 = d_pos1; a.valid1 = d_valid1; a.cands = d_cands; a.its_for_n = d_its_for_n;
    a.n_corr = d_n_corr; a.n_its = d_n_its; a.corr = d_corr; a.sets = d_sets; a.hyp = d_hyp; a.bits = d_inlier_bits; a.events = d_events;
    a.n_events = d_n_events; a.status = d_status;
    for (int k = 0; k < 12; k++) a.T1w[k] = T1w[k];
    // mvnMaxError1/2 are std::vector<size_t> (include/Sim3Solver.h:78-79): 9.210 * sigmaSquare is truncated, then compared as a float
    for (int l = 0; l < ORBFE_MAX_LEVELS; l++) a.gate[l] = l < cp->nlevels ? (float)(size_t)(9.210 * (double)ctx->plan.sigma2[l]) : 0.f;
    a.fx = cp->fx; a.fy = cp->fy; a.cx = cp->cx; a.cy = cp->cy;
    a.n1 = n1; a.nlevels = cp->nlevels; a.max_pairs = max_pairs; a.max_kf_n = max_kf_n;
    a.cap = (max_pairs + 3) & ~3;
    a.words = (max_pairs + 31) / 32;
    a.fix_scale = fix_scale != 0; a.min_inliers = min_inliers; a.max_its = max_its;
    if (ctx->sim3_ransac_scratch.ensure(sizeof(float) * SR_FIELDS * (size_t)a.cap * n_cands)) return orbfe_fail(ctx, ORBFE_ERR_HIP, "Sim3 RANSAC scratch allocation failed");
    a.table = (float *)ctx->sim3_ransac_scratch.p;
    hipLaunchKernelGGL(sim3_filter_kernel, dim3(n_cands), dim3(SR_THREADS), 0, s, a);
    const dim3 grid((max_its + SR_HPW - 1) / SR_HPW, n_cands);
    if (max_pairs <= ORBFE_SIM3_RANSAC_LDS_SLOTS) hipLaunchKernelGGL((sim3_hyp_kernel<true>), grid, dim3(64), hyp_lds_bytes(a.cap), s, a);
    else hipLaunchKernelGGL((sim3_hyp_kernel<false>), grid, dim3(64), hyp_lds_bytes(0), s, a);
    hipLaunchKernelGGL(sim3_events_kernel, dim3(n_cands), dim3(64), 0, s, a);
    ORBFE_HIP_TRY(ctx, hipGetLastError());
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

extern "C" int orbfe_enqueue_sim3_ransac_select(orbfe_context *ctx, const orbfe_sim3_ransac_candidate *d_cands, int n_cands, int c, int k, int kf1_n,
                                                const int32_t *d_valid1, int max_pairs, int max_kf_n, int max_its, const int32_t *d_n_corr,
                                                const int32_t *d_n_its, const int32_t *d_corr, const uint32_t *d_inlier_bits, int32_t *d_prior12,
                                                int32_t *d_valid1_round, int32_t *d_valid2_round, int32_t *d_status, void *stream)
try {
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    ORBFE_ENTRY(ctx);
    if (!d_cands || !d_n_corr || !d_n_its || !d_corr || !d_inlier_bits || !d_valid2_round || !d_status) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null argument");
    if (kf1_n < 0 || kf1_n > 65535 || max_kf_n < 0 || max_kf_n > 65535 || max_pairs < 1 || max_pairs > 65535)
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "kf1_n = %d, max_kf_n = %d (0 .. 65535), max_pairs = %d (1 .. 65535)", kf1_n, max_kf_n, max_pairs);
    if (kf1_n > 0 && (!d_valid1 || !d_prior12 || !d_valid1_round)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null array of keyframe 1");
    if (c < 0 || c >= n_cands || k < 0 || k >= max_its) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "candidate %d of %d, iteration %d of %d", c, n_cands, k, max_its);
    hipStream_t s;
    if (const int rc = orbfe_enqueue_on(ctx, stream, false, &s)) return rc;
    SelectArgs a;
    a.cands = d_cands; a.valid1 = d_valid1; a.n_corr = d_n_corr; a.n_its = d_n_its; a.corr = d_corr; a.bits = d_inlier_bits;
    a.prior12 = d_prior12; a.valid1_round = d_valid1_round; a.valid2_round = d_valid2_round; a.status = d_status;
    a.c = c; a.k = k; a.n1 = kf1_n; a.max_pairs = max_pairs; a.max_kf_n = max_kf_n; a.max_its = max_its; a.words = (max_pairs + 31) / 32;
    hipLaunchKernelGGL(sim3_select_kernel, dim3(1), dim3(SR_THREADS), 0, s, a);
    ORBFE_HIP_TRY(ctx, hipGetLastError());
    return ORBFE_OK;
} ORBFE_CATCH(ctx)

extern "C" int orbfe_sim3_ransac(orbfe_context *ctx, const orbfe_keypoint *keys_un1, int n1, const float *T1w, const float *pos1, const int32_t *valid1,
                                 const orbfe_keypoint *keys_un2, int n2, const float *T2w, const float *pos2, const int32_t *valid2, const int32_t *pairs,
                                 int n_pairs, const uint32_t *draws, int fix_scale, int min_inliers, int max_its, const int32_t *its_for_n, int *n_corr,
                                 int *n_its, int32_t *corr, int32_t *sets, orbfe_sim3_hypothesis *hyp, uint32_t *inlier_bits, int32_t *events, int *n_events)
try {
    if (!ctx) return orbfe_fail(nullptr, ORBFE_ERR_INVALID, "null context");
    ORBFE_ENTRY(ctx);
    if (!T1w || !T2w || !draws || !its_for_n || !n_corr || !n_its || !corr || !hyp || !inlier_bits || !events || !n_events)
        return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null argument");
    if (n1 < 0 || n1 > 65535 || n2 < 0 || n2 > 65535) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "keyframe with %d / %d keypoints (0 .. 65535)", n1, n2);
    if (n_pairs < 0 || n_pairs > 65535 || (n_pairs > 0 && !pairs)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "n_pairs = %d (0 .. 65535) or a null pair array", n_pairs);
    if (n1 > 0 && (!keys_un1 || !pos1 || !valid1)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null array of keyframe 1");
    if (n2 > 0 && (!keys_un2 || !pos2 || !valid2)) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "null array of keyframe 2");
    if (min_inliers < 3 || max_its < 1 || max_its > 65536) return orbfe_fail(ctx, ORBFE_ERR_INVALID, "min_inliers = %d (>= 3), max_its = %d (1 .. 65536)", min_inliers, max_its);
    hipStream_t s;
    if (const int rc = orbfe_enqueue_on(ctx, nullptr, false, &s)) return rc;
    const int max_pairs = std::max(n_pairs, 1), max_kf_n = std::max(n1, n2), words = (max_pairs + 31) / 32;
    // the staging block: results first, then the inputs
    const size_t its = (size_t)max_its;
    orbfe::StageLayout L;
    const auto f_cnt = L.result<int32_t>(4); // n_corr, n_its, n_events, status
    const auto f_corr = L.result<int32_t>(max_pairs, 2); const auto f_sets = L.result<int32_t>(its, 3); const auto f_hyp = L.result<orbfe_sim3_hypothesis>(its);
    const auto f_bits = L.result<uint32_t>(its, words); const auto f_ev = L.result<int32_t>(its);
    const auto f_rec = L.input<orbfe_sim3_ransac_candidate>(1);
    const auto f_np = L.input<int32_t>(1); const auto f_T2 = L.input<float>(12); const auto f_k1 = L.input<orbfe_keypoint>(n1);
    const auto f_k2 = L.input<orbfe_keypoint>(n2); const auto f_p1 = L.input<float>(n1, 3); const auto f_p2 = L.input<float>(n2, 3);
    const auto f_v1 = L.input<int32_t>(n1); const auto f_v2 = L.input<int32_t>(n2); const auto f_pairs = L.input<int32_t>(n_pairs, 2);
    const auto f_draws = L.input<uint32_t>(its, 3); const auto f_tab = L.input<int32_t>((size_t)max_pairs + 1);
    if (ctx->sync_stage.ensure(L.bytes())) return orbfe_fail(ctx, ORBFE_ERR_HIP, "Sim3 RANSAC staging allocation failed");
    StageBlock blk(L, ctx->sync_stage);
    blk.put(f_k1, keys_un1, n1); blk.put(f_p1, pos1, 3 * (size_t)n1); blk.put(f_v1, valid1, n1);
    blk.put(f_k2, keys_un2, n2); blk.put(f_p2, pos2, 3 * (size_t)n2); blk.put(f_v2, valid2, n2); blk.put(f_pairs, pairs, 2 * (size_t)n_pairs);
    blk.put(f_draws, draws, 3 * its); blk.put(f_tab, its_for_n, (size_t)n_pairs + 1); // the table covers N <= n_pairs; with n_pairs == 0 its entry 1 is never read
    blk.put(f_T2, T2w, 12);
    const int32_t np32 = n_pairs;
    blk.put(f_np, &np32, 1);
    orbfe_sim3_ransac_candidate rec = {};
    rec.keys_un = blk.dev(f_k2); rec.pos = blk.dev(f_p2); rec.valid = blk.dev(f_v2); rec.T2w = blk.dev(f_T2); rec.pairs = blk.dev(f_pairs);
    rec.n_pairs = blk.dev(f_np); rec.draws = blk.dev(f_draws); rec.n = n2;
    blk.put(f_rec, &rec, 1);
    ORBFE_HIP_TRY(ctx, blk.upload(s));
    orbfe_grid_keyframe kf1 = {}; // only keys_un and n are read
    kf1.keys_un = blk.dev(f_k1); kf1.n = n1;
    int32_t *cnt = blk.dev(f_cnt);
    const int rc = orbfe_enqueue_sim3_ransac_batch(ctx, &kf1, T1w, blk.dev(f_p1), blk.dev(f_v1), blk.dev(f_rec), 1, max_pairs, max_kf_n, fix_scale, min_inliers, max_its,
                                                   blk.dev(f_tab), cnt, cnt + 1, blk.dev(f_corr), blk.dev(f_sets), blk.dev(f_hyp), blk.dev(f_bits), blk.dev(f_ev),
                                                   cnt + 2, cnt + 3, nullptr);
    if (rc != ORBFE_OK) return rc;
    ORBFE_HIP_TRY(ctx, blk.download(s));
    ORBFE_HIP_TRY(ctx, hipStreamSynchronize(s));
    int32_t c4[4];
    blk.get(f_cnt, c4, 4);
    *n_corr = c4[0]; *n_its = c4[1]; *n_events = c4[2];
    blk.get(f_corr, corr, f_corr.count);
    if (sets) blk.get(f_sets, sets, f_sets.count);
    blk.get(f_hyp, hyp, f_hyp.count); blk.get(f_bits, inlier_bits, f_bits.count); blk.get(f_ev, events, f_ev.count);
    if (c4[3] != 0) return orbfe_fail(ctx, c4[3], "a pair index out of range or a keypoint octave outside the context's %d levels", ctx->params.nlevels);
    return ORBFE_OK;
} ORBFE_CATCH(ctx)
