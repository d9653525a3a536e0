// PnPsolver.h -- the PnPsolver port (reference src/PnPsolver.cc): the iteration table and the draw rows that
// orbfe_enqueue_pnp_ransac_batch takes, EPnP and CheckInliers as the contract states them, the literal host form of every row the
// kernels write, and ORB_SLAM2::PnPsolver, which answers the reference's SetRansacParameters / iterate / find from the rows of either
// backend -- the host form below or the rows fetched from the device.  Header-only, no OpenCV, no device needed.
//
// The arithmetic (everything marked ORBFE_CV_HD, down to PnPDrawSet) is ONE definition: orbfe_pnp_ransac.hip includes this header and
// compiles the same functions for gfx950, one lane per EPnP, so a kernel and the host form cannot differ in an operation or in an
// order.  tests/pnp_solver_model.py is the second, independent formulation; tests/pnp_solver_mirror/mirror_main.cpp is the driver that
// compares the two bit for bit.  Compile with -ffp-contract=off, as CvMat.h asks.
//
// A correspondence set is never copied: EPnP's loops over pws / us / alphas / pcs walk the correspondence table through a PnPSet (four
// drawn indices, or the set bits of an inlier row), and alphas and pcs, which the reference stores per point, are recomputed where they
// are read -- the same expressions on the same operands, hence the same bits.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/orbfe.h"
#include "CvMat.h"

namespace ORB_SLAM2
{

// ---------------------------------------------------------------------------------------------------------------- draws
// DUtils::Random::RandomInt(0, d - 1) on a raw value (Thirdparty/DLib/src/Random.cpp:47-50; RAND_MAX = 2^31 - 1)
ORBFE_CV_HD inline int PnPRandomInt(uint32_t r, int d) { return (int)(((double)r / 2147483648.0) * d); }

// the four correspondences of :189-202: vAvailableIndices starts as 0 .. N-1 and each draw swaps with the back and pops.  Only drawn
// positions ever differ from the identity, so at most four overrides stand for the vector.  N >= 4.
ORBFE_CV_HD inline void PnPDrawSet(const uint32_t r[4], int N, int32_t ids[4])
{
    int pos[4], val[4], n = 0;
    for (int i = 0; i < 4; i++) {
        const int size = N - i;
        int randi = PnPRandomInt(r[i], size);
        if (randi > size - 1) randi = size - 1; // a raw value above RAND_MAX cannot index beyond the vector
        int at = randi, back = size - 1;
        for (int q = 0; q < n; q++) {
            if (pos[q] == randi) at = val[q];
            if (pos[q] == size - 1) back = val[q];
        }
        ids[i] = at;
        int q = 0;
        while (q < n && pos[q] != randi) q++;
        pos[q] = randi; val[q] = back;
        if (q == n) n++;
    }
}

// ---------------------------------------------------------------------------------------------------------------- EPnP
struct PnPCamera { double fu, fv, uc, vc; }; // fu = F.fx ...: doubles that hold floats (:105-108)

struct PnPTable { // per correspondence, as the constructor leaves them (:88-97): mvP3Dw, mvP2D, mvMaxError
    const float *X, *Y, *Z, *u, *v, *max_error;
};

// the correspondences of one compute_pose: ids[0 .. 3] (a drawn set), or, with ids == NULL, the set bits of bits[0 .. range) in
// ascending order (an inlier row); n = number_of_correspondences
struct PnPSet {
    const int32_t *ids;
    const uint32_t *bits;
    int range, n;
};

ORBFE_CV_HD inline bool PnPSetHas(const PnPSet &S, int j) { return S.ids ? true : ((S.bits[j >> 5] >> (j & 31)) & 1u) != 0; }
ORBFE_CV_HD inline int PnPSetIndex(const PnPSet &S, int j) { return S.ids ? S.ids[j] : j; }

struct PnPWork { // what compute_pose keeps between its steps
    double cws[4][3], ccs[4][3], cc_inv[9], ut[144], l_6x10[60], rho[6];
};

ORBFE_CV_HD inline double PnPDot(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

ORBFE_CV_HD inline double PnPDist2(const double *p1, const double *p2)
{
    return (p1[0] - p2[0]) * (p1[0] - p2[0]) + (p1[1] - p2[1]) * (p1[1] - p2[1]) + (p1[2] - p2[2]) * (p1[2] - p2[2]);
}

// add_correspondence (:364-374): floats widened
ORBFE_CV_HD inline void PnPPoint(const PnPTable &T, int idx, double pw[3], double us[2])
{
    pw[0] = T.X[idx]; pw[1] = T.Y[idx]; pw[2] = T.Z[idx];
    us[0] = T.u[idx]; us[1] = T.v[idx];
}

// one row of compute_barycentric_coordinates (:424-434)
ORBFE_CV_HD inline void PnPAlphas(const PnPWork &w, const double pi[3], double a[4])
{
    const double *ci = w.cc_inv;
    for (int j = 0; j < 3; j++)
        a[1 + j] = ci[3 * j] * (pi[0] - w.cws[0][0]) + ci[3 * j + 1] * (pi[1] - w.cws[0][1]) + ci[3 * j + 2] * (pi[2] - w.cws[0][2]);
    a[0] = 1.0 - a[1] - a[2] - a[3]; // 1.0f is widened
}

// choose_control_points (:376-410)
ORBFE_CV_HD inline void PnPChooseControlPoints(const PnPTable &T, const PnPSet &S, PnPWork &w)
{
    double pw[3], us[2];
    w.cws[0][0] = w.cws[0][1] = w.cws[0][2] = 0;
    for (int q = 0; q < S.range; q++) {
        if (!PnPSetHas(S, q)) continue;
        PnPPoint(T, PnPSetIndex(S, q), pw, us);
        for (int j = 0; j < 3; j++) w.cws[0][j] += pw[j];
    }
    for (int j = 0; j < 3; j++) w.cws[0][j] /= S.n;
    double pw0tpw0[9], dc[3], uct[9], row[3];
    for (int k = 0; k < 9; k++) pw0tpw0[k] = 0;
    for (int q = 0; q < S.range; q++) {
        if (!PnPSetHas(S, q)) continue;
        PnPPoint(T, PnPSetIndex(S, q), pw, us);
        for (int j = 0; j < 3; j++) row[j] = pw[j] - w.cws[0][j];
        MulTransposedAdd(pw0tpw0, row, 3);
    }
    MulTransposedMirror(pw0tpw0, 3);
    SvdSquareD(pw0tpw0, 3, dc, uct, nullptr);
    for (int i = 1; i < 4; i++) {
        const double k = std::sqrt(dc[i - 1] / S.n);
        for (int j = 0; j < 3; j++) w.cws[i][j] = w.cws[0][j] + k * uct[3 * (i - 1) + j];
    }
}

// compute_L_6x10 (:761-801)
ORBFE_CV_HD inline void PnPComputeL6x10(const double *ut, double *l_6x10)
{
    const double *v[4] = {ut + 12 * 11, ut + 12 * 10, ut + 12 * 9, ut + 12 * 8};
    double dv[4][6][3];
    for (int i = 0; i < 4; i++) {
        int a = 0, b = 1;
        for (int j = 0; j < 6; j++) {
            dv[i][j][0] = v[i][3 * a] - v[i][3 * b];
            dv[i][j][1] = v[i][3 * a + 1] - v[i][3 * b + 1];
            dv[i][j][2] = v[i][3 * a + 2] - v[i][3 * b + 2];
            b++;
            if (b > 3) { a++; b = a + 1; }
        }
    }
    for (int i = 0; i < 6; i++) {
        double *row = l_6x10 + 10 * i;
        row[0] = PnPDot(dv[0][i], dv[0][i]);
        row[1] = 2.0 * PnPDot(dv[0][i], dv[1][i]);
        row[2] = PnPDot(dv[1][i], dv[1][i]);
        row[3] = 2.0 * PnPDot(dv[0][i], dv[2][i]);
        row[4] = 2.0 * PnPDot(dv[1][i], dv[2][i]);
        row[5] = PnPDot(dv[2][i], dv[2][i]);
        row[6] = 2.0 * PnPDot(dv[0][i], dv[3][i]);
        row[7] = 2.0 * PnPDot(dv[1][i], dv[3][i]);
        row[8] = 2.0 * PnPDot(dv[2][i], dv[3][i]);
        row[9] = PnPDot(dv[3][i], dv[3][i]);
    }
}

// find_betas_approx_1 / _2 / _3 (:668-759); which = 1, 2, 3
ORBFE_CV_HD inline void PnPFindBetasApprox(int which, const double *l_6x10, const double *rho, double *betas)
{
    const int cols1[4] = {0, 1, 3, 6};
    const int n = which == 1 ? 4 : which == 2 ? 3 : 5;
    double L[30], b[5], sv[5];
    for (int i = 0; i < 6; i++)
        for (int c = 0; c < n; c++) L[i * n + c] = l_6x10[10 * i + (which == 1 ? cols1[c] : c)];
    SolveSvdD(L, 6, n, rho, b, sv);
    if (which == 1) {
        if (b[0] < 0) {
            betas[0] = std::sqrt(-b[0]);
            betas[1] = -b[1] / betas[0];
            betas[2] = -b[2] / betas[0];
            betas[3] = -b[3] / betas[0];
        } else {
            betas[0] = std::sqrt(b[0]);
            betas[1] = b[1] / betas[0];
            betas[2] = b[2] / betas[0];
            betas[3] = b[3] / betas[0];
        }
        return;
    }
    if (b[0] < 0) {
        betas[0] = std::sqrt(-b[0]);
        betas[1] = (b[2] < 0) ? std::sqrt(-b[2]) : 0.0;
    } else {
        betas[0] = std::sqrt(b[0]);
        betas[1] = (b[2] > 0) ? std::sqrt(b[2]) : 0.0;
    }
    if (b[1] < 0) betas[0] = -betas[0];
    betas[2] = which == 3 ? b[3] / betas[0] : 0.0;
    betas[3] = 0.0;
}

// qr_solve (:861-951) of the 6 x 4 system; its eta == 0 exit leaves X as it was
ORBFE_CV_HD inline void PnPQrSolve(double *pA, double *pb, double *pX)
{
    const int nr = 6, nc = 4;
    double A1[6], A2[6];
    double *ppAkk = pA;
    for (int k = 0; k < nc; k++) {
        double *ppAik = ppAkk, eta = std::fabs(*ppAik);
        for (int i = k + 1; i < nr; i++) {
            const double elt = std::fabs(*ppAik);
            if (eta < elt) eta = elt;
            ppAik += nc;
        }
        if (eta == 0) return;
        double sum = 0.0;
        const double inv_eta = 1. / eta;
        ppAik = ppAkk;
        for (int i = k; i < nr; i++) {
            *ppAik *= inv_eta;
            sum += *ppAik * *ppAik;
            ppAik += nc;
        }
        double sigma = std::sqrt(sum);
        if (*ppAkk < 0) sigma = -sigma;
        *ppAkk += sigma;
        A1[k] = sigma * *ppAkk;
        A2[k] = -eta * sigma;
        for (int j = k + 1; j < nc; j++) {
            double *p = ppAkk, s = 0;
            for (int i = k; i < nr; i++) {
                s += *p * p[j - k];
                p += nc;
            }
            const double tau = s / A1[k];
            p = ppAkk;
            for (int i = k; i < nr; i++) {
                p[j - k] -= tau * *p;
                p += nc;
            }
        }
        ppAkk += nc + 1;
    }
    double *ppAjj = pA;
    for (int j = 0; j < nc; j++) { // b <- Qt b
        double *ppAij = ppAjj, tau = 0;
        for (int i = j; i < nr; i++) {
            tau += *ppAij * pb[i];
            ppAij += nc;
        }
        tau /= A1[j];
        ppAij = ppAjj;
        for (int i = j; i < nr; i++) {
            pb[i] -= tau * *ppAij;
            ppAij += nc;
        }
        ppAjj += nc + 1;
    }
    pX[nc - 1] = pb[nc - 1] / A2[nc - 1]; // X = R-1 b
    for (int i = nc - 2; i >= 0; i--) {
        const double *ppAij = pA + i * nc + (i + 1);
        double sum = 0;
        for (int j = i + 1; j < nc; j++) {
            sum += *ppAij * pX[j];
            ppAij++;
        }
        pX[i] = (pb[i] - sum) / A2[i];
    }
}

// gauss_newton (:841-859) with compute_A_and_b_gauss_newton (:813-839); x is zero before the first solve (the reference's is not set)
ORBFE_CV_HD inline void PnPGaussNewton(const double *l_6x10, const double *rho, double betas[4])
{
    double a[24], b[6], x[4] = {0, 0, 0, 0};
    for (int k = 0; k < 5; k++) {
        for (int i = 0; i < 6; i++) {
            const double *rowL = l_6x10 + i * 10;
            double *rowA = a + i * 4;
            rowA[0] = 2 * rowL[0] * betas[0] + rowL[1] * betas[1] + rowL[3] * betas[2] + rowL[6] * betas[3];
            rowA[1] = rowL[1] * betas[0] + 2 * rowL[2] * betas[1] + rowL[4] * betas[2] + rowL[7] * betas[3];
            rowA[2] = rowL[3] * betas[0] + rowL[4] * betas[1] + 2 * rowL[5] * betas[2] + rowL[8] * betas[3];
            rowA[3] = rowL[6] * betas[0] + rowL[7] * betas[1] + rowL[8] * betas[2] + 2 * rowL[9] * betas[3];
            b[i] = rho[i] - (rowL[0] * betas[0] * betas[0] + rowL[1] * betas[0] * betas[1] + rowL[2] * betas[1] * betas[1] + rowL[3] * betas[0] * betas[2] +
                             rowL[4] * betas[1] * betas[2] + rowL[5] * betas[2] * betas[2] + rowL[6] * betas[0] * betas[3] + rowL[7] * betas[1] * betas[3] +
                             rowL[8] * betas[2] * betas[3] + rowL[9] * betas[3] * betas[3]);
        }
        PnPQrSolve(a, b, x);
        for (int i = 0; i < 4; i++) betas[i] += x[i];
    }
}

// one row of compute_pcs (:467-476)
ORBFE_CV_HD inline void PnPPc(const PnPWork &w, const double a[4], double pc[3])
{
    for (int j = 0; j < 3; j++) pc[j] = a[0] * w.ccs[0][j] + a[1] * w.ccs[1][j] + a[2] * w.ccs[2][j] + a[3] * w.ccs[3][j];
}

// compute_R_and_t (:652-663): compute_ccs, compute_pcs, solve_for_sign, estimate_R_and_t, reprojection_error
ORBFE_CV_HD inline double PnPComputeRAndT(const PnPTable &T, const PnPSet &S, const PnPCamera &cam, PnPWork &w, const double *betas, double R[3][3], double t[3])
{
    double pw[3], us[2], a[4], pc[3];
    for (int i = 0; i < 4; i++) w.ccs[i][0] = w.ccs[i][1] = w.ccs[i][2] = 0.0;
    for (int i = 0; i < 4; i++) {
        const double *v = w.ut + 12 * (11 - i);
        for (int j = 0; j < 4; j++)
            for (int k = 0; k < 3; k++) w.ccs[j][k] += betas[i] * v[3 * j + k];
    }
    // solve_for_sign (:637-650) looks at pcs[2], the depth of the FIRST point; negating ccs before pcs is formed negates every pc exactly
    for (int q = 0; q < S.range; q++) {
        if (!PnPSetHas(S, q)) continue;
        PnPPoint(T, PnPSetIndex(S, q), pw, us);
        PnPAlphas(w, pw, a);
        PnPPc(w, a, pc);
        if (pc[2] < 0.0)
            for (int i = 0; i < 4; i++)
                for (int j = 0; j < 3; j++) w.ccs[i][j] = -w.ccs[i][j];
        break;
    }
    // estimate_R_and_t (:570-628)
    double pc0[3] = {0, 0, 0}, pw0[3] = {0, 0, 0};
    for (int q = 0; q < S.range; q++) {
        if (!PnPSetHas(S, q)) continue;
        PnPPoint(T, PnPSetIndex(S, q), pw, us);
        PnPAlphas(w, pw, a);
        PnPPc(w, a, pc);
        for (int j = 0; j < 3; j++) { pc0[j] += pc[j]; pw0[j] += pw[j]; }
    }
    for (int j = 0; j < 3; j++) { pc0[j] /= S.n; pw0[j] /= S.n; }
    double abt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, abt_w[3], abt_ut[9], abt_vt[9];
    for (int q = 0; q < S.range; q++) {
        if (!PnPSetHas(S, q)) continue;
        PnPPoint(T, PnPSetIndex(S, q), pw, us);
        PnPAlphas(w, pw, a);
        PnPPc(w, a, pc);
        for (int j = 0; j < 3; j++) {
            abt[3 * j] += (pc[j] - pc0[j]) * (pw[0] - pw0[0]);
            abt[3 * j + 1] += (pc[j] - pc0[j]) * (pw[1] - pw0[1]);
            abt[3 * j + 2] += (pc[j] - pc0[j]) * (pw[2] - pw0[2]);
        }
    }
    SvdSquareD(abt, 3, abt_w, abt_ut, abt_vt);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) // dot(abt_u + 3 * i, abt_v + 3 * j) on U and V, whose columns are the rows of Ut and Vt
            R[i][j] = abt_ut[i] * abt_vt[j] + abt_ut[3 + i] * abt_vt[3 + j] + abt_ut[6 + i] * abt_vt[6 + j];
    const double det = R[0][0] * R[1][1] * R[2][2] + R[0][1] * R[1][2] * R[2][0] + R[0][2] * R[1][0] * R[2][1] - R[0][2] * R[1][1] * R[2][0] -
                       R[0][1] * R[1][0] * R[2][2] - R[0][0] * R[1][2] * R[2][1];
    if (det < 0) {
        R[2][0] = -R[2][0];
        R[2][1] = -R[2][1];
        R[2][2] = -R[2][2];
    }
    t[0] = pc0[0] - PnPDot(R[0], pw0);
    t[1] = pc0[1] - PnPDot(R[1], pw0);
    t[2] = pc0[2] - PnPDot(R[2], pw0);
    // reprojection_error (:551-568)
    double sum2 = 0.0;
    for (int q = 0; q < S.range; q++) {
        if (!PnPSetHas(S, q)) continue;
        PnPPoint(T, PnPSetIndex(S, q), pw, us);
        const double Xc = PnPDot(R[0], pw) + t[0];
        const double Yc = PnPDot(R[1], pw) + t[1];
        const double inv_Zc = 1.0 / (PnPDot(R[2], pw) + t[2]);
        const double ue = cam.uc + cam.fu * Xc * inv_Zc;
        const double ve = cam.vc + cam.fv * Yc * inv_Zc;
        sum2 += std::sqrt((us[0] - ue) * (us[0] - ue) + (us[1] - ve) * (us[1] - ve));
    }
    return sum2 / S.n;
}

// compute_pose (:478-526)
ORBFE_CV_HD inline double PnPComputePose(const PnPTable &T, const PnPSet &S, const PnPCamera &cam, PnPWork &w, double R[3][3], double t[3])
{
    double pw[3], us[2], a[4], cc[9], cc_w[3];
    PnPChooseControlPoints(T, S, w);
    for (int i = 0; i < 3; i++) // compute_barycentric_coordinates (:412-435)
        for (int j = 1; j < 4; j++) cc[3 * i + j - 1] = w.cws[j][i] - w.cws[0][i];
    InvertSvd3D(cc, w.cc_inv, cc_w);
    double mtm[144], d[12], M1[12], M2[12];
    for (int k = 0; k < 144; k++) mtm[k] = 0;
    for (int q = 0; q < S.range; q++) { // fill_M (:437-452), two rows at a time into cvMulTransposed
        if (!PnPSetHas(S, q)) continue;
        PnPPoint(T, PnPSetIndex(S, q), pw, us);
        PnPAlphas(w, pw, a);
        for (int i = 0; i < 4; i++) {
            M1[3 * i] = a[i] * cam.fu;
            M1[3 * i + 1] = 0.0;
            M1[3 * i + 2] = a[i] * (cam.uc - us[0]);
            M2[3 * i] = 0.0;
            M2[3 * i + 1] = a[i] * cam.fv;
            M2[3 * i + 2] = a[i] * (cam.vc - us[1]);
        }
        MulTransposedAdd(mtm, M1, 12);
        MulTransposedAdd(mtm, M2, 12);
    }
    MulTransposedMirror(mtm, 12);
    SvdSquareD(mtm, 12, d, w.ut, nullptr);
    PnPComputeL6x10(w.ut, w.l_6x10);
    w.rho[0] = PnPDist2(w.cws[0], w.cws[1]); // compute_rho (:803-811)
    w.rho[1] = PnPDist2(w.cws[0], w.cws[2]);
    w.rho[2] = PnPDist2(w.cws[0], w.cws[3]);
    w.rho[3] = PnPDist2(w.cws[1], w.cws[2]);
    w.rho[4] = PnPDist2(w.cws[1], w.cws[3]);
    w.rho[5] = PnPDist2(w.cws[2], w.cws[3]);
    double Betas[4][4], rep_errors[4], Rs[4][3][3], ts[4][3];
    for (int which = 1; which <= 3; which++) {
        PnPFindBetasApprox(which, w.l_6x10, w.rho, Betas[which]);
        PnPGaussNewton(w.l_6x10, w.rho, Betas[which]);
        rep_errors[which] = PnPComputeRAndT(T, S, cam, w, Betas[which], Rs[which], ts[which]);
    }
    int N = 1;
    if (rep_errors[2] < rep_errors[1]) N = 2;
    if (rep_errors[3] < rep_errors[N]) N = 3;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) R[i][j] = Rs[N][i][j];
        t[i] = ts[N][i];
    }
    return rep_errors[N];
}

// one correspondence of CheckInliers (:309-340), with its mixed widths
ORBFE_CV_HD inline bool PnPIsInlier(const PnPTable &T, int i, const PnPCamera &cam, const double R[3][3], const double t[3])
{
    const double x = T.X[i], y = T.Y[i], z = T.Z[i];
    const float Xc = (float)(R[0][0] * x + R[0][1] * y + R[0][2] * z + t[0]);
    const float Yc = (float)(R[1][0] * x + R[1][1] * y + R[1][2] * z + t[1]);
    const float invZc = (float)(1 / (R[2][0] * x + R[2][1] * y + R[2][2] * z + t[2]));
    const double ue = cam.uc + cam.fu * Xc * invZc;
    const double ve = cam.vc + cam.fv * Yc * invZc;
    const float distX = (float)(T.u[i] - ue);
    const float distY = (float)(T.v[i] - ve);
    const float error2 = distX * distX + distY * distY;
    return error2 < T.max_error[i]; // a NaN fails
}

// mRansacMinInliers after SetRansacParameters (:135-140) for N correspondences
ORBFE_CV_HD inline int PnPMinInliers(int N, int minInliers, float epsilon)
{
    int nMinInliers = (int)((float)N * epsilon);
    if (nMinInliers < minInliers) nMinInliers = minInliers;
    if (nMinInliers < 4) nMinInliers = 4;
    return nMinInliers;
}

// ---------------------------------------------------------------------------------------------------------------- table
// SetRansacParameters (:122-158) for N correspondences: mRansacMaxIts afterwards; 0 stands for the N < mRansacMinInliers exit of iterate
// (:174-178).  The reference's quirks stay: pow(epsilon, 3) although the minimal set is 4, the int truncation of N * epsilon, the float
// epsilon bump.
inline int PnPRansacIterations(int N, double prob, int minInliers, int maxIts, float epsilon)
{
    const int nMin = PnPMinInliers(N, minInliers, epsilon);
    if (N < nMin) return 0;
    float eps = epsilon;
    if (eps < (float)nMin / N) eps = (float)nMin / N;
    double n;
    if (nMin == N) n = 1;
    else n = std::ceil(std::log(1 - prob) / std::log(1 - std::pow((double)eps, 3.0)));
    const int nIterations = !(n < maxIts) ? maxIts : (int)n; // the clamp before the conversion: no overflow
    return std::max(1, std::min(nIterations, maxIts));
}

// d_its_for_n of orbfe_enqueue_pnp_ransac_batch: one entry per N in [0, capacity]
inline std::vector<int32_t> PnPRansacIterationTable(int capacity, double prob, int minInliers, int maxIts, float epsilon)
{
    std::vector<int32_t> t((size_t)capacity + 1);
    for (int N = 0; N <= capacity; N++) t[N] = PnPRansacIterations(N, prob, minInliers, maxIts, epsilon);
    return t;
}

// a draw row [maxIts][4] of raw rand() values, as DUtils::Random::RandomInt consumes them
inline void DrawPnPSets(uint32_t *draws, int maxIts)
{
    for (int k = 0; k < 4 * maxIts; k++) draws[k] = (uint32_t)rand();
}

// ---------------------------------------------------------------------------------------------------------------- the host form
struct PnPRows { // the rows of one candidate, as the device writes them
    int32_t status = 0, n_corr = 0, n_its = 0, n_events = 0, exhausted = -1;
    int capacity = 0, max_its = 0, words = 0;
    std::vector<int32_t> corr, sets, events;                 // [capacity][2], [max_its][4], [max_its]
    std::vector<orbfe_pnp_hypothesis> hyp;                   // [max_its]
    std::vector<orbfe_pnp_refined> refined;                  // [max_its]
    std::vector<uint32_t> bits, refined_bits;                // [max_its][words]
};

// the rows of candidate c as fetched from the device after orbfe_enqueue_pnp_ransac_batch (host copies of its output arrays, all
// candidates).  corr and the two bit arrays may be NULL when they were not downloaded: iterate() then reports no inlier flags.
inline PnPRows PnPRowsOfCandidate(int c, int capacity, int max_its, const int32_t *status, const int32_t *n_corr, const int32_t *n_its, const int32_t *n_events,
                                  const int32_t *exhausted, const int32_t *events, const orbfe_pnp_hypothesis *hyp, const orbfe_pnp_refined *refined,
                                  const int32_t *corr, const uint32_t *bits, const uint32_t *refined_bits)
{
    PnPRows o;
    o.status = status ? status[c] : 0; o.n_corr = n_corr[c]; o.n_its = n_its[c]; o.n_events = n_events[c]; o.exhausted = exhausted[c];
    o.capacity = capacity; o.max_its = max_its; o.words = (capacity + 31) / 32;
    const size_t rows = (size_t)max_its * o.words;
    o.events.assign(events + (size_t)c * max_its, events + (size_t)(c + 1) * max_its);
    o.sets.assign((size_t)4 * max_its, -1); // the drawn sets are not needed to walk the rows
    o.hyp.assign(hyp + (size_t)c * max_its, hyp + (size_t)(c + 1) * max_its);
    o.refined.assign(refined + (size_t)c * max_its, refined + (size_t)(c + 1) * max_its);
    if (corr) o.corr.assign(corr + (size_t)c * 2 * capacity, corr + (size_t)(c + 1) * 2 * capacity);
    else o.corr.assign((size_t)2 * capacity, -1);
    if (bits) o.bits.assign(bits + c * rows, bits + (c + 1) * rows);
    else o.bits.assign(rows, 0u);
    if (refined_bits) o.refined_bits.assign(refined_bits + c * rows, refined_bits + (c + 1) * rows);
    else o.refined_bits.assign(rows, 0u);
    return o;
}

struct PnPProblem { // the constructor's vectors (:68-111) and the parameters of SetRansacParameters
    std::vector<float> X, Y, Z, u, v, max_error;
    std::vector<int32_t> corr; // (frame keypoint, keyframe slot) per correspondence
    PnPCamera cam;
    int min_inliers = 0; // mRansacMinInliers after the adjustment
    PnPTable table() const { return PnPTable{X.data(), Y.data(), Z.data(), u.data(), v.data(), max_error.data()}; }
    int N() const { return (int)X.size(); }
};

// the constructor's filter on flat arrays.  cam = fx, fy, cx, cy.  Returns the status.
inline int PnPFilter(const orbfe_keypoint *keys_un, int n_keys, const int32_t *f_match, const float *pos, const int32_t *valid, int n_kf, const float *sigma2,
                     int nlevels, const float cam[4], float th2, PnPProblem &P)
{
    int status = 0;
    P.cam = PnPCamera{cam[0], cam[1], cam[2], cam[3]};
    for (int i = 0; i < n_keys; i++) {
        const int m = f_match[i];
        if (m == -1) continue;
        if (m < -1 || m >= n_kf || keys_un[i].octave < 0 || keys_un[i].octave >= nlevels) { status = ORBFE_ERR_INVALID; continue; }
        if (!valid[m]) continue;
        P.X.push_back(pos[3 * (size_t)m]); P.Y.push_back(pos[3 * (size_t)m + 1]); P.Z.push_back(pos[3 * (size_t)m + 2]);
        P.u.push_back(keys_un[i].x); P.v.push_back(keys_un[i].y);
        P.max_error.push_back(sigma2[keys_un[i].octave] * th2);
        P.corr.push_back(i); P.corr.push_back(m);
    }
    return status;
}

inline void PnPStorePose(const double R[3][3], const double t[3], float *Rout, float *tout, int tstride)
{
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) Rout[(tstride ? 4 : 3) * i + j] = Stored((float)R[i][j]);
        tout[tstride ? 4 * i : i] = Stored((float)t[i]);
    }
}

// CheckInliers over all correspondences into a bit row; returns mnInliersi
inline int PnPCheckInliers(const PnPProblem &P, const double R[3][3], const double t[3], uint32_t *row)
{
    const PnPTable T = P.table();
    int count = 0;
    for (int j = 0; j < P.N(); j++)
        if (PnPIsInlier(T, j, P.cam, R, t)) {
            row[j >> 5] |= 1u << (j & 31);
            count++;
        }
    return count;
}

// iteration k of iterate (:185-208) from its four raw draws, into the rows
inline void PnPHypothesisHost(const PnPProblem &P, const uint32_t raw[4], int k, PnPRows &o)
{
    int32_t *ids = &o.sets[4 * (size_t)k];
    PnPDrawSet(raw, P.N(), ids);
    const PnPSet S = {ids, nullptr, 4, 4};
    PnPWork w;
    double R[3][3], t[3];
    PnPComputePose(P.table(), S, P.cam, w, R, t);
    orbfe_pnp_hypothesis &H = o.hyp[k];
    H.n_inliers = PnPCheckInliers(P, R, t, &o.bits[(size_t)k * o.words]);
    PnPStorePose(R, t, H.Rcw, H.tcw, 0);
}

// Refine() (:261-306) on the inliers of hypothesis k, into the rows
inline void PnPRefineHost(const PnPProblem &P, int k, PnPRows &o)
{
    const PnPSet S = {nullptr, &o.bits[(size_t)k * o.words], P.N(), o.hyp[k].n_inliers};
    PnPWork w;
    double R[3][3], t[3];
    PnPComputePose(P.table(), S, P.cam, w, R, t);
    orbfe_pnp_refined &F = o.refined[k];
    F.n_inliers = PnPCheckInliers(P, R, t, &o.refined_bits[(size_t)k * o.words]);
    F.ok = F.n_inliers > P.min_inliers;
    PnPStorePose(R, t, F.Tcw, F.Tcw + 3, 1);
}

inline void PnPRowsInit(PnPRows &o, int capacity, int max_its)
{
    o.capacity = capacity; o.max_its = max_its; o.words = (capacity + 31) / 32;
    o.corr.assign((size_t)2 * capacity, -1);
    o.sets.assign((size_t)4 * max_its, -1);
    o.events.assign(max_its, -1);
    o.hyp.assign(max_its, orbfe_pnp_hypothesis());
    for (auto &h : o.hyp) h.best_k = -1;
    o.refined.assign(max_its, orbfe_pnp_refined());
    o.bits.assign((size_t)max_its * o.words, 0u);
    o.refined_bits.assign((size_t)max_its * o.words, 0u);
}

// every row of orbfe_enqueue_pnp_ransac_batch for one candidate, computed on the host.  P (may be NULL) receives the problem, for a
// solver that is to continue beyond the rows.
inline PnPRows PnPRansacHost(const orbfe_keypoint *keys_un, int n_keys, const int32_t *f_match, const float *pos, const int32_t *valid, int n_kf,
                             const uint32_t *draws, int capacity, int min_inliers, int max_its, int n_iterations, float epsilon, float th2,
                             const int32_t *its_for_n, const float *sigma2, int nlevels, const float cam[4], PnPProblem *problem = nullptr)
{
    PnPRows o;
    PnPRowsInit(o, capacity, max_its);
    PnPProblem P;
    if (n_keys < 0 || n_keys > capacity || n_kf < 0) { o.status = ORBFE_ERR_INVALID; return o; }
    o.status = PnPFilter(keys_un, n_keys, f_match, pos, valid, n_kf, sigma2, nlevels, cam, th2, P);
    const int N = P.N();
    P.min_inliers = PnPMinInliers(N, min_inliers, epsilon);
    o.n_corr = N;
    std::memcpy(o.corr.data(), P.corr.data(), sizeof(int32_t) * P.corr.size());
    o.n_its = its_for_n[N] <= 0 || N < 4 ? 0 : std::min(max_its, std::max(its_for_n[N], n_iterations));
    int best = 0, best_k = -1; // mnBestInliers starts at 0
    for (int k = 0; k < o.n_its; k++) {
        PnPHypothesisHost(P, draws + 4 * (size_t)k, k, o);
        const int count = o.hyp[k].n_inliers;
        if (count >= P.min_inliers) {
            if (count > best) {
                best = count; best_k = k;
                PnPRefineHost(P, k, o);
            }
            if (o.refined[best_k].ok) o.events[o.n_events++] = k;
        }
        o.hyp[k].best_k = best_k;
    }
    o.exhausted = best_k;
    if (problem) *problem = P;
    return o;
}

// ---------------------------------------------------------------------------------------------------------------- the reference's class
// The reference's interface on stored rows.  The rows -- of PnPRansacHost or fetched from the device -- hold the first n_its iterations,
// which is all that the first iterate(nIterations) call can run when the rows were made with n_iterations >= nIterations.  Because of the
// `||` in the loop condition (:183) a call made AFTER a success runs nIterations further iterations whatever mRansacMaxIts is, so a
// solver can be asked for iterations beyond its rows.  It then continues with the host form on the problem given to the constructor,
// with fresh rand() draws, as the reference would; without a problem the end of the rows counts as exhaustion (bNoMore, mBestTcw if any).
class PnPsolver
{
public:
    enum { kNone = -1, kBest = -2 }; // iterate's return besides an event's iteration: an empty cv::Mat; mBestTcw on exhaustion

    // its_for_n_N: the iteration table's entry for the rows' n_corr (mRansacMaxIts); n_keys: the frame's keypoints (vbInliers' size)
    PnPsolver(const PnPRows *rows, int n_keys, int its_for_n_N, int minInliers, float epsilon, const PnPProblem *problem = nullptr)
        : mRows(*rows), mProblem(problem), mNKeys(n_keys)
    {
        N = mRows.n_corr;
        mRansacMinInliers = PnPMinInliers(N, minInliers, epsilon);
        mRansacMaxIts = its_for_n_N;
        mBestK = -1;
        mnBestInliers = 0;
        mnIterations = 0;
    }

    int iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers)
    {
        bNoMore = false;
        vbInliers.clear();
        nInliers = 0;
        mPose = nullptr;
        if (N < mRansacMinInliers || mRansacMaxIts <= 0) {
            bNoMore = true;
            return kNone;
        }
        int nCurrentIterations = 0;
        bool ended = false;
        while (mnIterations < mRansacMaxIts || nCurrentIterations < nIterations) {
            const int k = mnIterations;
            if (k >= mRows.n_its && !Continue(k)) { // the rows end and there is nothing to continue with: treated as exhaustion
                ended = true;
                break;
            }
            nCurrentIterations++;
            mnIterations++;
            const int count = mRows.hyp[k].n_inliers;
            if (count >= mRansacMinInliers) {
                if (count > mnBestInliers) { mnBestInliers = count; mBestK = k; }
                const orbfe_pnp_refined &F = mRows.refined[mBestK];
                if (F.ok) {
                    nInliers = F.n_inliers;
                    Flags(&mRows.refined_bits[(size_t)mBestK * mRows.words], vbInliers);
                    mPose = F.Tcw;
                    return k;
                }
            }
        }
        if (ended || mnIterations >= mRansacMaxIts) {
            bNoMore = true;
            if (mnBestInliers >= mRansacMinInliers) {
                nInliers = mnBestInliers;
                Flags(&mRows.bits[(size_t)mBestK * mRows.words], vbInliers);
                const orbfe_pnp_hypothesis &H = mRows.hyp[mBestK];
                for (int i = 0; i < 3; i++) {
                    for (int j = 0; j < 3; j++) mBestTcw[4 * i + j] = H.Rcw[3 * i + j];
                    mBestTcw[4 * i + 3] = H.tcw[i];
                }
                mPose = mBestTcw;
                return kBest;
            }
        }
        return kNone;
    }

    int find(std::vector<bool> &vbInliers, int &nInliers)
    {
        bool bFlag;
        return iterate(mRansacMaxIts, bFlag, vbInliers, nInliers);
    }

    const float *GetPose() const { return mPose; } // 3 x 4 row-major, of what iterate returned last; NULL after kNone
    int Iterations() const { return mnIterations; }
    int BestIteration() const { return mBestK; }

private:
    void Flags(const uint32_t *bits, std::vector<bool> &vbInliers) const
    {
        vbInliers = std::vector<bool>(mNKeys, false);
        for (int i = 0; i < N; i++)
            if ((bits[i >> 5] >> (i & 31)) & 1u) {
                const int kp = mRows.corr[2 * (size_t)i];
                if (kp >= 0 && kp < mNKeys) vbInliers[kp] = true;
            }
    }

    // iteration k beyond the stored rows, appended to the solver's own copy of them
    bool Continue(int k)
    {
        if (!mProblem || mProblem->N() != N || N < 4) return false;
        while ((int)mRows.hyp.size() <= k) {
            const size_t at = mRows.hyp.size();
            orbfe_pnp_hypothesis h = orbfe_pnp_hypothesis();
            h.best_k = -1;
            mRows.hyp.push_back(h);
            mRows.refined.push_back(orbfe_pnp_refined());
            mRows.sets.resize(4 * (at + 1), -1);
            mRows.bits.resize((at + 1) * mRows.words, 0u);
            mRows.refined_bits.resize((at + 1) * mRows.words, 0u);
        }
        uint32_t raw[4];
        DrawPnPSets(raw, 1);
        PnPHypothesisHost(*mProblem, raw, k, mRows);
        if (mRows.hyp[k].n_inliers >= mRansacMinInliers && mRows.hyp[k].n_inliers > mnBestInliers) PnPRefineHost(*mProblem, k, mRows);
        mRows.n_its = k + 1;
        return true;
    }

    PnPRows mRows; // a copy: a continuation appends to it
    const PnPProblem *mProblem;
    int mNKeys, N = 0, mRansacMinInliers = 0, mRansacMaxIts = 0, mnIterations = 0, mnBestInliers = 0, mBestK = -1;
    const float *mPose = nullptr;
    float mBestTcw[12] = {};
};

} // namespace ORB_SLAM2
