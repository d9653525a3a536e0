/*
 * orb_oracle.c -- CPU ORACLE (test infrastructure, NOT product code).
 * See orb_oracle.h for the provenance statement (PARITY UNPINNED).
 *
 * Build: gcc -O2 -std=c11 -ffp-contract=off -fno-fast-math -shared -fPIC
 * Floating point: every float expression below is written so that it is
 * evaluated in IEEE binary32/binary64 with one rounding per operation
 * (contract Q4 of SURVEY.md: no FMA contraction).
 */
#include "orb_oracle.h"

#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

/* ------------------------------------------------------------------ */
/* scalar helpers                                                      */
/* ------------------------------------------------------------------ */

/* OPENCV-4.5.5-SEMANTICS cvRound: cvtss2si / lrint, round-half-to-even. */
int orc_cv_round_f(float v) { return (int)lrintf(v); }
int orc_cv_round_d(double v) { return (int)lrint(v); }

/* OPENCV-4.5.5-SEMANTICS cv::fastAtan2 scalar path (mathfuncs_core: atan_f32);
 * called at reference src/ORBextractor.cc:98. */
float orc_fast_atan2(float y, float x)
{
    const float k = (float)(180.0 / 3.14159265358979323846);
    const float p1 = 0.9997878412794807f * k;
    const float p3 = -0.3258083974640975f * k;
    const float p5 = 0.1555786518463281f * k;
    const float p7 = -0.04432655554792128f * k;
    const float eps = (float)DBL_EPSILON;
    float ax = fabsf(x), ay = fabsf(y);
    float a, c, c2;
    if (ax >= ay) {
        c = ay / (ax + eps);
        c2 = c * c;
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    } else {
        c = ax / (ay + eps);
        c2 = c * c;
        a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    }
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a;
}

/* Contract Q4: cos/sin of the keypoint angle are produced by ONE
 * deterministic routine shared (as an algorithm) by this oracle and the HIP
 * kernels: double-precision argument reduction by pi/2 and the classic
 * fdlibm-style kernel polynomials, rounded once to float.  The reference calls
 * libm cosf/sinf (src/ORBextractor.cc:108); this routine equals the correctly
 * rounded value except on near-tie inputs (tests measure the mismatch rate
 * against libm). Valid for rad in [-1, 8]. */
void orc_sincos_det(float rad, float *s, float *c)
{
    static const double TWO_OVER_PI = 6.36619772367581382433e-01;
    static const double PIO2_HI = 1.57079632673412561417e+00; /* 33 bits */
    static const double PIO2_LO = 6.07710050650619224932e-11;
    static const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03,
                        S3 = -1.98412698298579493134e-04, S4 = 2.75573137070700676789e-06,
                        S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    static const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03,
                        C3 = 2.48015872894767294178e-05, C4 = -2.75573143513906633035e-07,
                        C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    double x = (double)rad;
    double t = x * TWO_OVER_PI + 0.5;
    int q = (int)t;
    if (t < 0.0 && (double)q != t) q -= 1; /* floor */
    double qd = (double)q;
    double r = (x - qd * PIO2_HI) - qd * PIO2_LO;
    double z = r * r;
    double sp = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
    double sr = r + (z * r) * (S1 + z * sp);
    double cp = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))));
    double cr = 1.0 - (0.5 * z - z * cp);
    double sv, cv;
    switch (q & 3) {
    case 0: sv = sr; cv = cr; break;
    case 1: sv = cr; cv = -sr; break;
    case 2: sv = -sr; cv = -cr; break;
    default: sv = -cr; cv = sr; break;
    }
    *s = (float)sv;
    *c = (float)cv;
}

/* OPENCV-4.5.5-SEMANTICS borderInterpolate(p, len, BORDER_REFLECT_101) */
int orc_border_reflect101(int p, int len)
{
    if (len == 1) return 0;
    while (p < 0 || p >= len) {
        if (p < 0) p = -p;
        else p = 2 * len - 2 - p;
    }
    return p;
}

/* Array forms of the three scalar helpers above: plain loops over the scalar routines, for tests that feed millions of inputs
 * (tests/test_arith_blocks.py).  s and c of orc_sincos_det_n may not alias. */
void orc_fast_atan2_n(const float *y, const float *x, float *out, size_t n)
{
    for (size_t i = 0; i < n; ++i) out[i] = orc_fast_atan2(y[i], x[i]);
}

void orc_sincos_det_n(const float *rad, float *s, float *c, size_t n)
{
    for (size_t i = 0; i < n; ++i) orc_sincos_det(rad[i], &s[i], &c[i]);
}

void orc_border_reflect101_n(const int32_t *p, const int32_t *len, int32_t *out, size_t n)
{
    for (size_t i = 0; i < n; ++i) out[i] = orc_border_reflect101(p[i], len[i]);
}

/* ORBmatcher::DescriptorDistance, reference src/ORBmatcher.cc:1643-1659:
 * SWAR popcount over 8 x uint32 == plain 256-bit Hamming distance. */
int orc_hamming256(const uint8_t *a, const uint8_t *b)
{
    int dist = 0;
    for (int i = 0; i < 8; i++) {
        uint32_t pa, pb;
        memcpy(&pa, a + 4 * i, 4);
        memcpy(&pb, b + 4 * i, 4);
        uint32_t v = pa ^ pb;
        v = v - ((v >> 1) & 0x55555555u);
        v = (v & 0x33333333u) + ((v >> 2) & 0x33333333u);
        dist += (int)((((v + (v >> 4)) & 0xF0F0F0Fu) * 0x1010101u) >> 24);
    }
    return dist;
}

static const int32_t g_bit_pattern_31[256 * 4] = {
#include "../orbslam2_amd/csrc/orb_pattern_31.inc"
};

const int32_t *orc_bit_pattern(void) { return g_bit_pattern_31; }

/* OPENCV-4.5.5-SEMANTICS getGaussianKernelBitExact + getGaussianKernelFixedPoint_ED
 * (smooth.dispatch.cpp): normalised Gaussian, then 1/256 units with error
 * diffusion from the outside in; centre tap absorbs the remainder. */
void orc_gaussian_taps_q8(int ksize, double sigma, int32_t *taps)
{
    double g[64];
    double scale2x = -0.5 / (sigma * sigma);
    double sum = 0.0;
    for (int i = 0; i < ksize; i++) {
        double x = (double)i - (double)(ksize - 1) * 0.5;
        g[i] = exp(scale2x * x * x);
        sum += g[i];
    }
    sum = 1.0 / sum;
    for (int i = 0; i < ksize; i++) g[i] *= sum;
    int n2 = ksize / 2;
    double err = 0.0;
    int64_t acc = 0;
    for (int i = 0; i < n2; i++) {
        double adj = g[i] * 256.0 + err;
        int64_t v0 = (int64_t)lrint(adj);
        err = adj - (double)v0;
        taps[i] = (int32_t)v0;
        taps[ksize - 1 - i] = (int32_t)v0;
        acc += 2 * v0;
    }
    taps[n2] = (int32_t)(256 - acc);
}

/* ------------------------------------------------------------------ */
/* cv::resize, 8UC1, INTER_LINEAR                                      */
/* ------------------------------------------------------------------ */

static short sat_short_from_float(float v)
{
    int r = (int)lrintf(v);
    if (r > SHRT_MAX) r = SHRT_MAX;
    if (r < SHRT_MIN) r = SHRT_MIN;
    return (short)r;
}

/* OPENCV-4.5.5-SEMANTICS resize.cpp: resizeGeneric_<HResizeLinear<uchar,int,short,2048>,
 * VResizeLinear<uchar,int,short,FixedPtCast<int,uchar,22>>>; called at reference
 * src/ORBextractor.cc:934 with dsize given (fx=fy=0). */
void orc_resize_linear_u8(const uint8_t *src, int sw, int sh, size_t sstride,
                          uint8_t *dst, int dw, int dh, size_t dstride)
{
    double inv_scale_x = (double)dw / (double)sw;
    double inv_scale_y = (double)dh / (double)sh;
    double scale_x = 1.0 / inv_scale_x, scale_y = 1.0 / inv_scale_y;

    int *xofs = (int *)malloc(sizeof(int) * (size_t)dw);
    short *alpha = (short *)malloc(sizeof(short) * 2 * (size_t)dw);
    int *rows0 = (int *)malloc(sizeof(int) * (size_t)dw);
    int *rows1 = (int *)malloc(sizeof(int) * (size_t)dw);

    for (int dx = 0; dx < dw; dx++) {
        float fx = (float)(((double)dx + 0.5) * scale_x - 0.5);
        int sx = (int)floorf(fx);
        fx -= (float)sx;
        if (sx < 0) { fx = 0.f; sx = 0; }
        if (sx >= sw - 1) { fx = 0.f; sx = sw - 1; }
        xofs[dx] = sx;
        alpha[2 * dx] = sat_short_from_float((1.f - fx) * 2048.f);
        alpha[2 * dx + 1] = sat_short_from_float(fx * 2048.f);
    }
    for (int dy = 0; dy < dh; dy++) {
        float fy = (float)(((double)dy + 0.5) * scale_y - 0.5);
        int sy = (int)floorf(fy);
        fy -= (float)sy;
        short b0 = sat_short_from_float((1.f - fy) * 2048.f);
        short b1 = sat_short_from_float(fy * 2048.f);
        int sy0 = sy < 0 ? 0 : (sy > sh - 1 ? sh - 1 : sy);
        int sy1 = sy + 1 < 0 ? 0 : (sy + 1 > sh - 1 ? sh - 1 : sy + 1);
        const uint8_t *S0 = src + (size_t)sy0 * sstride;
        const uint8_t *S1 = src + (size_t)sy1 * sstride;
        for (int dx = 0; dx < dw; dx++) {
            int sx = xofs[dx];
            int sx1 = sx + 1 < sw ? sx + 1 : sw - 1; /* weight is 0 when clamped */
            rows0[dx] = S0[sx] * alpha[2 * dx] + S0[sx1] * alpha[2 * dx + 1];
            rows1[dx] = S1[sx] * alpha[2 * dx] + S1[sx1] * alpha[2 * dx + 1];
        }
        uint8_t *D = dst + (size_t)dy * dstride;
        for (int dx = 0; dx < dw; dx++) {
            int v = (((b0 * (rows0[dx] >> 4)) >> 16) + ((b1 * (rows1[dx] >> 4)) >> 16) + 2) >> 2;
            D[dx] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
        }
    }
    free(xofs); free(alpha); free(rows0); free(rows1);
}

/* ------------------------------------------------------------------ */
/* cv::GaussianBlur(7x7, sigma 2, REFLECT_101), 8UC1 fixed point       */
/* ------------------------------------------------------------------ */

/* OPENCV-4.5.5-SEMANTICS smooth.simd.hpp fixedSmoothInvoker<uint8_t, ufixedpoint16>:
 * row pass in 8.8 (uint16), column pass to 16.16 with +2^15 >> 16 rounding.
 * Called at reference src/ORBextractor.cc:899-900 on a clone (not a sub-matrix). */
void orc_gaussian7_u8(const uint8_t *src, int w, int h, size_t sstride,
                      uint8_t *dst, size_t dstride)
{
    int32_t k[7];
    orc_gaussian_taps_q8(7, 2.0, k);
    uint16_t *tmp = (uint16_t *)malloc(sizeof(uint16_t) * (size_t)w * (size_t)h);
    for (int y = 0; y < h; y++) {
        const uint8_t *S = src + (size_t)y * sstride;
        for (int x = 0; x < w; x++) {
            uint32_t acc = 0;
            for (int i = 0; i < 7; i++) {
                int xx = orc_border_reflect101(x + i - 3, w);
                acc += (uint32_t)k[i] * S[xx];
            }
            tmp[(size_t)y * w + x] = (uint16_t)acc; /* <= 255*256 */
        }
    }
    for (int y = 0; y < h; y++) {
        uint8_t *D = dst + (size_t)y * dstride;
        for (int x = 0; x < w; x++) {
            uint32_t acc = 0;
            for (int j = 0; j < 7; j++) {
                int yy = orc_border_reflect101(y + j - 3, h);
                acc += (uint32_t)k[j] * tmp[(size_t)yy * w + x];
            }
            uint32_t v = (acc + (1u << 15)) >> 16;
            D[x] = (uint8_t)(v > 255 ? 255 : v);
        }
    }
    free(tmp);
}

/* ------------------------------------------------------------------ */
/* cv::FAST 9_16                                                       */
/* ------------------------------------------------------------------ */

static const int g_ring_dx[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
static const int g_ring_dy[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};

static void make_ring_offsets(ptrdiff_t pixel[25], size_t stride)
{
    for (int k = 0; k < 16; k++) pixel[k] = g_ring_dx[k] + g_ring_dy[k] * (ptrdiff_t)stride;
    for (int k = 16; k < 25; k++) pixel[k] = pixel[k - 16];
}

/* OPENCV-4.5.5-SEMANTICS fast_score.cpp cornerScore<16> */
static int corner_score16(const uint8_t *ptr, const ptrdiff_t pixel[25], int threshold)
{
    int d[25];
    int v = ptr[0];
    for (int k = 0; k < 25; k++) d[k] = (short)(v - ptr[pixel[k]]);
    int a0 = threshold;
    for (int k = 0; k < 16; k += 2) {
        int a = d[k + 1] < d[k + 2] ? d[k + 1] : d[k + 2];
        if (d[k + 3] < a) a = d[k + 3];
        if (a <= a0) continue;
        for (int m = 4; m <= 8; m++) if (d[k + m] < a) a = d[k + m];
        int t = a < d[k] ? a : d[k];
        if (t > a0) a0 = t;
        t = a < d[k + 9] ? a : d[k + 9];
        if (t > a0) a0 = t;
    }
    int b0 = -a0;
    for (int k = 0; k < 16; k += 2) {
        int b = d[k + 1] > d[k + 2] ? d[k + 1] : d[k + 2];
        for (int m = 3; m <= 5; m++) if (d[k + m] > b) b = d[k + m];
        if (b >= b0) continue;
        for (int m = 6; m <= 8; m++) if (d[k + m] > b) b = d[k + m];
        int t = b > d[k] ? b : d[k];
        if (t < b0) b0 = t;
        t = b > d[k + 9] ? b : d[k + 9];
        if (t < b0) b0 = t;
    }
    return -b0 - 1;
}

int orc_fast_corner_score(const uint8_t *ptr, size_t stride, int threshold)
{
    ptrdiff_t pixel[25];
    make_ring_offsets(pixel, stride);
    return corner_score16(ptr, pixel, threshold);
}

int orc_fast_score_closed_form(const uint8_t *ptr, size_t stride, int threshold)
{
    int d[16];
    int v = ptr[0];
    for (int k = 0; k < 16; k++)
        d[k] = v - ptr[g_ring_dx[k] + g_ring_dy[k] * (ptrdiff_t)stride];
    int best = threshold;
    for (int s = 0; s < 16; s++) {
        int mn = INT_MAX, mx = INT_MIN;
        for (int m = 0; m < 9; m++) {
            int dv = d[(s + m) & 15];
            if (dv < mn) mn = dv;
            if (dv > mx) mx = dv;
        }
        if (mn > best) best = mn;     /* dark arc: all v-p >= mn */
        if (-mx > best) best = -mx;   /* bright arc: all p-v >= -mx */
    }
    return best - 1;
}

/* OPENCV-4.5.5-SEMANTICS fast.cpp FAST_t<16> (scalar path); called at reference
 * src/ORBextractor.cc:803,808 on cell sub-matrices. */
int orc_fast9_16(const uint8_t *img, int w, int h, size_t stride, int threshold,
                 int nonmax, int32_t *xs, int32_t *ys, int32_t *scores, int cap)
{
    const int K = 8, N = 25;
    int count_out = 0;
    if (w < 7 || h < 7) return 0;
    ptrdiff_t pixel[25];
    make_ring_offsets(pixel, stride);
    if (threshold < 0) threshold = 0;
    if (threshold > 255) threshold = 255;
    uint8_t tab[512];
    for (int i = -255; i <= 255; i++)
        tab[i + 255] = (uint8_t)(i < -threshold ? 1 : (i > threshold ? 2 : 0));

    uint8_t *buf[3];
    int *cpbuf[3];
    for (int i = 0; i < 3; i++) {
        buf[i] = (uint8_t *)calloc((size_t)w, 1);
        cpbuf[i] = (int *)calloc((size_t)w + 1, sizeof(int));
    }
    for (int i = 3; i < h - 2; i++) {
        const uint8_t *ptr = img + (size_t)i * stride + 3;
        uint8_t *curr = buf[(i - 3) % 3];
        int *cornerpos = cpbuf[(i - 3) % 3] + 1;
        memset(curr, 0, (size_t)w);
        int ncorners = 0;
        if (i < h - 3) {
            for (int j = 3; j < w - 3; j++, ptr++) {
                int v = ptr[0];
                const uint8_t *t = &tab[0] - v + 255;
                int d = t[ptr[pixel[0]]] | t[ptr[pixel[8]]];
                if (d == 0) continue;
                d &= t[ptr[pixel[2]]] | t[ptr[pixel[10]]];
                d &= t[ptr[pixel[4]]] | t[ptr[pixel[12]]];
                d &= t[ptr[pixel[6]]] | t[ptr[pixel[14]]];
                if (d == 0) continue;
                d &= t[ptr[pixel[1]]] | t[ptr[pixel[9]]];
                d &= t[ptr[pixel[3]]] | t[ptr[pixel[11]]];
                d &= t[ptr[pixel[5]]] | t[ptr[pixel[13]]];
                d &= t[ptr[pixel[7]]] | t[ptr[pixel[15]]];
                if (d & 1) {
                    int vt = v - threshold, count = 0;
                    for (int k = 0; k < N; k++) {
                        int x = ptr[pixel[k]];
                        if (x < vt) {
                            if (++count > K) {
                                cornerpos[ncorners++] = j;
                                if (nonmax) curr[j] = (uint8_t)corner_score16(ptr, pixel, threshold);
                                break;
                            }
                        } else
                            count = 0;
                    }
                }
                if (d & 2) {
                    int vt = v + threshold, count = 0;
                    for (int k = 0; k < N; k++) {
                        int x = ptr[pixel[k]];
                        if (x > vt) {
                            if (++count > K) {
                                cornerpos[ncorners++] = j;
                                if (nonmax) curr[j] = (uint8_t)corner_score16(ptr, pixel, threshold);
                                break;
                            }
                        } else
                            count = 0;
                    }
                }
            }
        }
        cornerpos[-1] = ncorners;
        if (i == 3) continue;
        const uint8_t *prev = buf[(i - 4 + 3) % 3];
        const uint8_t *pprev = buf[(i - 5 + 3) % 3];
        cornerpos = cpbuf[(i - 4 + 3) % 3] + 1;
        ncorners = cornerpos[-1];
        for (int k = 0; k < ncorners; k++) {
            int j = cornerpos[k];
            int score = prev[j];
            if (!nonmax ||
                (score > prev[j + 1] && score > prev[j - 1] &&
                 score > pprev[j - 1] && score > pprev[j] && score > pprev[j + 1] &&
                 score > curr[j - 1] && score > curr[j] && score > curr[j + 1])) {
                if (count_out < cap) {
                    xs[count_out] = j;
                    ys[count_out] = i - 1;
                    scores[count_out] = score;
                }
                count_out++;
            }
        }
    }
    for (int i = 0; i < 3; i++) { free(buf[i]); free(cpbuf[i]); }
    return count_out;
}

/* ------------------------------------------------------------------ */
/* DistributeOctTree                                                   */
/* ------------------------------------------------------------------ */

typedef struct qnode {
    int x0, y0, x1, y1;   /* UL.x, UL.y, BR.x, BR.y (boxes stay axis aligned) */
    int *keys; int nkeys; /* candidate indices, original order preserved */
    int no_more;
    int prev, next;       /* std::list links (pool indices, -1 = none) */
    int seq;              /* creation sequence: stands in for the heap address (Q3) */
} qnode;

typedef struct qlist {
    qnode *pool; int npool, cappool;
    int head, tail, size;
    int next_seq;
} qlist;

static int ql_alloc(qlist *l)
{
    if (l->npool == l->cappool) {
        l->cappool = l->cappool ? l->cappool * 2 : 256;
        l->pool = (qnode *)realloc(l->pool, sizeof(qnode) * (size_t)l->cappool);
    }
    qnode *n = &l->pool[l->npool];
    memset(n, 0, sizeof(*n));
    n->prev = n->next = -1;
    n->seq = l->next_seq++;
    return l->npool++;
}
static void ql_push_back(qlist *l, int id)
{
    qnode *n = &l->pool[id];
    n->prev = l->tail; n->next = -1;
    if (l->tail >= 0) l->pool[l->tail].next = id; else l->head = id;
    l->tail = id; l->size++;
}
static void ql_push_front(qlist *l, int id)
{
    qnode *n = &l->pool[id];
    n->next = l->head; n->prev = -1;
    if (l->head >= 0) l->pool[l->head].prev = id; else l->tail = id;
    l->head = id; l->size++;
}
static int ql_erase(qlist *l, int id) /* returns next */
{
    qnode *n = &l->pool[id];
    int nx = n->next;
    if (n->prev >= 0) l->pool[n->prev].next = n->next; else l->head = n->next;
    if (n->next >= 0) l->pool[n->next].prev = n->prev; else l->tail = n->prev;
    l->size--;
    free(n->keys); n->keys = NULL; n->nkeys = 0;
    return nx;
}

/* ExtractorNode::DivideNode, reference src/ORBextractor.cc:475-531.  Children are
 * allocated in the pool (ids out[0..3]) but not linked. */
static void divide_node(qlist *l, int id, const int32_t *xs, const int32_t *ys, int out[4])
{
    int x0 = l->pool[id].x0, y0 = l->pool[id].y0, x1 = l->pool[id].x1, y1 = l->pool[id].y1;
    int nk = l->pool[id].nkeys;
    const int half_x = (int)ceilf((float)(x1 - x0) / 2);
    const int half_y = (int)ceilf((float)(y1 - y0) / 2);
    for (int c = 0; c < 4; c++) out[c] = ql_alloc(l);
    /* note: ql_alloc may move the pool; re-read pointers afterwards */
    qnode *n1 = &l->pool[out[0]], *n2 = &l->pool[out[1]], *n3 = &l->pool[out[2]], *n4 = &l->pool[out[3]];
    n1->x0 = x0;          n1->y0 = y0;          n1->x1 = x0 + half_x; n1->y1 = y0 + half_y;
    n2->x0 = x0 + half_x; n2->y0 = y0;          n2->x1 = x1;          n2->y1 = y0 + half_y;
    n3->x0 = x0;          n3->y0 = y0 + half_y; n3->x1 = x0 + half_x; n3->y1 = y1;
    n4->x0 = x0 + half_x; n4->y0 = y0 + half_y; n4->x1 = x1;          n4->y1 = y1;
    for (int c = 0; c < 4; c++) l->pool[out[c]].keys = (int *)malloc(sizeof(int) * (size_t)(nk > 0 ? nk : 1));
    const int *keys = l->pool[id].keys;
    const float midx = (float)(x0 + half_x), midy = (float)(y0 + half_y);
    for (int i = 0; i < nk; i++) {
        int k = keys[i];
        float px = (float)xs[k], py = (float)ys[k];
        qnode *dst;
        if (px < midx) dst = (py < midy) ? n1 : n3;
        else dst = (py < midy) ? n2 : n4;
        dst->keys[dst->nkeys++] = k;
    }
    for (int c = 0; c < 4; c++) if (l->pool[out[c]].nkeys == 1) l->pool[out[c]].no_more = 1;
}

typedef struct size_ptr { int size; int seq; int id; } size_ptr;
static int cmp_size_ptr(const void *a, const void *b)
{
    const size_ptr *p = (const size_ptr *)a, *q = (const size_ptr *)b;
    if (p->size != q->size) return p->size < q->size ? -1 : 1;
    if (p->seq != q->seq) return p->seq < q->seq ? -1 : 1; /* Q3: address order := creation order */
    return 0;
}

/* ORBextractor::DistributeOctTree, reference src/ORBextractor.cc:533-757.
 * Candidates carry integer coordinates (cv::FAST emits integer-valued floats).
 * Q3: the (size, pointer) sort key becomes (size, creation sequence). */
int orc_distribute_octtree(const int32_t *xs, const int32_t *ys, const int32_t *scores, int n,
                           int min_x, int max_x, int min_y, int max_y, int n_features,
                           int32_t *out_idx, int cap)
{
    qlist L; memset(&L, 0, sizeof(L)); L.head = L.tail = -1;
    int n_ini = (int)roundf((float)(max_x - min_x) / (float)(max_y - min_y));
    if (n_ini < 1) n_ini = 1; /* reference would index an empty vector (UB); documented guard */
    const float hX = (float)(max_x - min_x) / (float)n_ini;
    int *ini = (int *)malloc(sizeof(int) * (size_t)n_ini);
    for (int i = 0; i < n_ini; i++) {
        int id = ql_alloc(&L);
        qnode *nd = &L.pool[id];
        nd->x0 = (int)(hX * (float)i);
        nd->x1 = (int)(hX * (float)(i + 1));
        nd->y0 = 0;
        nd->y1 = max_y - min_y;
        nd->keys = (int *)malloc(sizeof(int) * (size_t)(n > 0 ? n : 1));
        ql_push_back(&L, id);
        ini[i] = id;
    }
    for (int i = 0; i < n; i++) {
        int b = (int)((float)xs[i] / hX);
        if (b < 0) b = 0;
        if (b >= n_ini) b = n_ini - 1; /* guard; unreachable for in-range points */
        qnode *nd = &L.pool[ini[b]];
        nd->keys[nd->nkeys++] = i;
    }
    free(ini);
    for (int it = L.head; it >= 0;) {
        qnode *nd = &L.pool[it];
        if (nd->nkeys == 1) { nd->no_more = 1; it = nd->next; }
        else if (nd->nkeys == 0) it = ql_erase(&L, it);
        else it = nd->next;
    }

    int finish = 0;
    size_ptr *vsp = NULL; int nvsp = 0, capvsp = 0;
    size_ptr *vprev = NULL; int capprev = 0;
#define VSP_PUSH(sz, idv) do { if (nvsp == capvsp) { capvsp = capvsp ? capvsp * 2 : 256; \
        vsp = (size_ptr *)realloc(vsp, sizeof(size_ptr) * (size_t)capvsp); } \
        vsp[nvsp].size = (sz); vsp[nvsp].id = (idv); vsp[nvsp].seq = L.pool[idv].seq; nvsp++; } while (0)

    while (!finish) {
        int prev_size = L.size;
        int n_to_expand = 0;
        nvsp = 0;
        for (int it = L.head; it >= 0;) {
            if (L.pool[it].no_more) { it = L.pool[it].next; continue; }
            int ch[4];
            divide_node(&L, it, xs, ys, ch);
            for (int c = 0; c < 4; c++) {
                if (L.pool[ch[c]].nkeys > 0) {
                    ql_push_front(&L, ch[c]);
                    if (L.pool[ch[c]].nkeys > 1) { n_to_expand++; VSP_PUSH(L.pool[ch[c]].nkeys, ch[c]); }
                } else { free(L.pool[ch[c]].keys); L.pool[ch[c]].keys = NULL; }
            }
            it = ql_erase(&L, it);
        }
        if (L.size >= n_features || L.size == prev_size) {
            finish = 1;
        } else if (L.size + n_to_expand * 3 > n_features) {
            while (!finish) {
                prev_size = L.size;
                if (nvsp > capprev) { capprev = nvsp; vprev = (size_ptr *)realloc(vprev, sizeof(size_ptr) * (size_t)capprev); }
                int nprev = nvsp;
                if (nprev) memcpy(vprev, vsp, sizeof(size_ptr) * (size_t)nprev);
                nvsp = 0;
                qsort(vprev, (size_t)nprev, sizeof(size_ptr), cmp_size_ptr);
                for (int j = nprev - 1; j >= 0; j--) {
                    int ch[4];
                    divide_node(&L, vprev[j].id, xs, ys, ch);
                    for (int c = 0; c < 4; c++) {
                        if (L.pool[ch[c]].nkeys > 0) {
                            ql_push_front(&L, ch[c]);
                            if (L.pool[ch[c]].nkeys > 1) VSP_PUSH(L.pool[ch[c]].nkeys, ch[c]);
                        } else { free(L.pool[ch[c]].keys); L.pool[ch[c]].keys = NULL; }
                    }
                    ql_erase(&L, vprev[j].id);
                    if (L.size >= n_features) break;
                }
                if (L.size >= n_features || L.size == prev_size) finish = 1;
            }
        }
    }
#undef VSP_PUSH
    int nout = 0;
    for (int it = L.head; it >= 0; it = L.pool[it].next) {
        const qnode *nd = &L.pool[it];
        int best = nd->keys[0];
        int max_resp = scores[best];
        for (int k = 1; k < nd->nkeys; k++) {
            if (scores[nd->keys[k]] > max_resp) { best = nd->keys[k]; max_resp = scores[best]; }
        }
        if (nout < cap) out_idx[nout] = best;
        nout++;
    }
    for (int i = 0; i < L.npool; i++) free(L.pool[i].keys);
    free(L.pool); free(vsp); free(vprev);
    return nout;
}

/* ------------------------------------------------------------------ */
/* orientation + descriptor                                            */
/* ------------------------------------------------------------------ */

/* IC_Angle, reference src/ORBextractor.cc:72-99 */
float orc_ic_angle(const uint8_t *img, size_t stride, int cx, int cy, const int32_t *umax, int half_patch)
{
    int m_01 = 0, m_10 = 0;
    const uint8_t *center = img + (size_t)cy * stride + cx;
    for (int u = -half_patch; u <= half_patch; ++u) m_10 += u * center[u];
    ptrdiff_t step = (ptrdiff_t)stride;
    for (int v = 1; v <= half_patch; ++v) {
        int v_sum = 0;
        int d = umax[v];
        for (int u = -d; u <= d; ++u) {
            int val_plus = center[u + v * step], val_minus = center[u - v * step];
            v_sum += (val_plus - val_minus);
            m_10 += u * (val_plus + val_minus);
        }
        m_01 += v * v_sum;
    }
    return orc_fast_atan2((float)m_01, (float)m_10);
}

/* computeOrbDescriptor, reference src/ORBextractor.cc:103-142.  cos/sin via the
 * contract routine (Q4); products and sums individually rounded. */
void orc_orb_descriptor_pat(const uint8_t *img, size_t stride, int cx, int cy, float angle_deg, const int32_t *pat, uint8_t *desc32)
{
    const float factor_pi = (float)(3.14159265358979323846 / (double)180.f);
    float angle = angle_deg * factor_pi;
    float a, b;
    orc_sincos_det(angle, &b, &a); /* a = cos, b = sin */
    const uint8_t *center = img + (size_t)cy * stride + cx;
    const ptrdiff_t step = (ptrdiff_t)stride;
    if (!pat) pat = g_bit_pattern_31;
    for (int i = 0; i < 32; i++) {
        int val = 0;
        for (int bit = 0; bit < 8; bit++, pat += 4) {
            float x0 = (float)pat[0], y0 = (float)pat[1], x1 = (float)pat[2], y1 = (float)pat[3];
            float r0a = x0 * b, r0b = y0 * a, c0a = x0 * a, c0b = y0 * b;
            float r1a = x1 * b, r1b = y1 * a, c1a = x1 * a, c1b = y1 * b;
            int t0 = center[orc_cv_round_f(r0a + r0b) * step + orc_cv_round_f(c0a - c0b)];
            int t1 = center[orc_cv_round_f(r1a + r1b) * step + orc_cv_round_f(c1a - c1b)];
            val |= (t0 < t1) << bit;
        }
        desc32[i] = (uint8_t)val;
    }
}

/* the compiled bit_pattern_31_ (src/ORBextractor.cc:145-403) */
void orc_orb_descriptor(const uint8_t *img, size_t stride, int cx, int cy, float angle_deg, uint8_t *desc32)
{
    orc_orb_descriptor_pat(img, stride, cx, cy, angle_deg, g_bit_pattern_31, desc32);
}

/* ------------------------------------------------------------------ */
/* extractor object                                                    */
/* ------------------------------------------------------------------ */

#define ORC_MAX_LEVELS 32

struct orc_extractor {
    orc_params p;
    double scale_factor_d; /* member is double, initialised from float (include/ORBextractor.h:96) */
    float scale[ORC_MAX_LEVELS], inv_scale[ORC_MAX_LEVELS], sigma2[ORC_MAX_LEVELS], inv_sigma2[ORC_MAX_LEVELS];
    int32_t feats[ORC_MAX_LEVELS];
    int32_t umax[64];
    int32_t pattern[256 * 4]; /* std::vector<cv::Point> pattern: the extractor's own copy of the 512 points (src/ORBextractor.cc:442-444) */
    /* state of the latest call */
    uint8_t *pyr[ORC_MAX_LEVELS];
    int lw[ORC_MAX_LEVELS], lh[ORC_MAX_LEVELS];
    int32_t *cx[ORC_MAX_LEVELS], *cy[ORC_MAX_LEVELS], *cs[ORC_MAX_LEVELS];
    int ncand[ORC_MAX_LEVELS];
};

/* ORBextractor::ORBextractor, reference src/ORBextractor.cc:405-464 */
orc_extractor *orc_extractor_create(const orc_params *p)
{
    if (!p || p->nlevels < 1 || p->nlevels > ORC_MAX_LEVELS || p->half_patch_size < 1 || p->half_patch_size > 62)
        return NULL;
    orc_extractor *ex = (orc_extractor *)calloc(1, sizeof(*ex));
    ex->p = *p;
    memcpy(ex->pattern, g_bit_pattern_31, sizeof(ex->pattern)); /* std::copy(pattern0, pattern0 + npoints, ...) :442-444 */
    ex->scale_factor_d = (double)p->scale_factor;
    ex->scale[0] = 1.0f; ex->sigma2[0] = 1.0f;
    for (int i = 1; i < p->nlevels; i++) {
        ex->scale[i] = (float)((double)ex->scale[i - 1] * ex->scale_factor_d);
        ex->sigma2[i] = ex->scale[i] * ex->scale[i];
    }
    for (int i = 0; i < p->nlevels; i++) {
        ex->inv_scale[i] = 1.0f / ex->scale[i];
        ex->inv_sigma2[i] = 1.0f / ex->sigma2[i];
    }
    float factor = (float)(1.0 / ex->scale_factor_d); /* 1.0f / double -> double -> float */
    float n_desired = (float)p->nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)p->nlevels));
    int sum = 0;
    for (int level = 0; level < p->nlevels - 1; level++) {
        ex->feats[level] = orc_cv_round_f(n_desired);
        sum += ex->feats[level];
        n_desired *= factor;
    }
    ex->feats[p->nlevels - 1] = p->nfeatures - sum > 0 ? p->nfeatures - sum : 0;

    int hp = p->half_patch_size;
    int vmax = (int)floor((double)((float)hp * sqrtf(2.f) / 2 + 1));
    int vmin = (int)ceil((double)((float)hp * sqrtf(2.f) / 2));
    const double hp2 = (double)(hp * hp);
    for (int v = 0; v <= vmax; ++v) ex->umax[v] = orc_cv_round_d(sqrt(hp2 - (double)(v * v)));
    for (int v = hp, v0 = 0; v >= vmin; --v) {
        while (ex->umax[v0] == ex->umax[v0 + 1]) ++v0;
        ex->umax[v] = v0;
        ++v0;
    }
    return ex;
}

static void free_state(orc_extractor *ex)
{
    for (int l = 0; l < ORC_MAX_LEVELS; l++) {
        free(ex->pyr[l]); ex->pyr[l] = NULL;
        free(ex->cx[l]); free(ex->cy[l]); free(ex->cs[l]);
        ex->cx[l] = ex->cy[l] = ex->cs[l] = NULL; ex->ncand[l] = 0;
        ex->lw[l] = ex->lh[l] = 0;
    }
}

void orc_extractor_destroy(orc_extractor *ex)
{
    if (!ex) return;
    free_state(ex);
    free(ex);
}

int orc_extractor_nlevels(const orc_extractor *ex) { return ex->p.nlevels; }
/* The reference's extractor owns a copy of the test pattern (member `pattern`, include/ORBextractor.h:93); a deployment that
 * distributes another table (BASELINE north_star: "broadcast of the ORB pattern") replaces it here: 256 tests x (x0, y0, x1, y1). */
void orc_extractor_set_pattern(orc_extractor *ex, const int32_t *pat1024) { memcpy(ex->pattern, pat1024, sizeof(ex->pattern)); }
const int32_t *orc_extractor_pattern(const orc_extractor *ex) { return ex->pattern; }
const float *orc_extractor_scale_factors(const orc_extractor *ex) { return ex->scale; }
const float *orc_extractor_inv_scale_factors(const orc_extractor *ex) { return ex->inv_scale; }
const float *orc_extractor_sigma2(const orc_extractor *ex) { return ex->sigma2; }
const float *orc_extractor_inv_sigma2(const orc_extractor *ex) { return ex->inv_sigma2; }
const int32_t *orc_extractor_features_per_level(const orc_extractor *ex) { return ex->feats; }
const int32_t *orc_extractor_umax(const orc_extractor *ex) { return ex->umax; }

/* level size, reference src/ORBextractor.cc:925-926 */
void orc_level_size(const orc_extractor *ex, int w, int h, int level, int *lw, int *lh)
{
    float s = ex->inv_scale[level];
    *lw = orc_cv_round_f((float)w * s);
    *lh = orc_cv_round_f((float)h * s);
}

const uint8_t *orc_pyramid_level(const orc_extractor *ex, int level, int *w, int *h, size_t *stride)
{
    if (level < 0 || level >= ex->p.nlevels || !ex->pyr[level]) return NULL;
    if (w) *w = ex->lw[level];
    if (h) *h = ex->lh[level];
    if (stride) *stride = (size_t)ex->lw[level];
    return ex->pyr[level];
}

int orc_level_candidates(const orc_extractor *ex, int level, const int32_t **xs, const int32_t **ys,
                         const int32_t **scores)
{
    if (level < 0 || level >= ex->p.nlevels) return -1;
    if (xs) *xs = ex->cx[level];
    if (ys) *ys = ex->cy[level];
    if (scores) *scores = ex->cs[level];
    return ex->ncand[level];
}

/* ORBextractor::ComputePyramid, reference src/ORBextractor.cc:921-946.  The
 * reflect-101 border ring the reference adds around each level is never read on
 * this path, so only the ROI pixels are kept. */
static void compute_pyramid(orc_extractor *ex, const uint8_t *img, int w, int h, size_t stride)
{
    for (int level = 0; level < ex->p.nlevels; ++level) {
        int lw, lh;
        orc_level_size(ex, w, h, level, &lw, &lh);
        ex->lw[level] = lw; ex->lh[level] = lh;
        ex->pyr[level] = (uint8_t *)malloc((size_t)(lw > 0 ? lw : 1) * (size_t)(lh > 0 ? lh : 1));
        if (level == 0) {
            for (int y = 0; y < h; y++) memcpy(ex->pyr[0] + (size_t)y * lw, img + (size_t)y * stride, (size_t)w);
        } else {
            orc_resize_linear_u8(ex->pyr[level - 1], ex->lw[level - 1], ex->lh[level - 1], (size_t)ex->lw[level - 1],
                                 ex->pyr[level], lw, lh, (size_t)lw);
        }
    }
}

static void cand_push(orc_extractor *ex, int level, int *capc, int x, int y, int s)
{
    if (ex->ncand[level] == *capc) {
        *capc = *capc ? *capc * 2 : 4096;
        ex->cx[level] = (int32_t *)realloc(ex->cx[level], sizeof(int32_t) * (size_t)*capc);
        ex->cy[level] = (int32_t *)realloc(ex->cy[level], sizeof(int32_t) * (size_t)*capc);
        ex->cs[level] = (int32_t *)realloc(ex->cs[level], sizeof(int32_t) * (size_t)*capc);
    }
    int n = ex->ncand[level]++;
    ex->cx[level][n] = x; ex->cy[level][n] = y; ex->cs[level][n] = s;
}

/* Cell-wise FAST of ComputeKeyPointsOctTree, reference src/ORBextractor.cc:759-825 */
static void level_candidates(orc_extractor *ex, int level)
{
    const float W = 30;
    const int et = ex->p.edge_threshold;
    const int lw = ex->lw[level], lh = ex->lh[level];
    const int min_bx = et - 3, min_by = min_bx;
    const int max_bx = lw - et + 3, max_by = lh - et + 3;
    const float width = (float)(max_bx - min_bx);
    const float height = (float)(max_by - min_by);
    const int n_cols = (int)(width / W);
    const int n_rows = (int)(height / W);
    int capc = 0;
    ex->ncand[level] = 0;
    if (n_cols < 1 || n_rows < 1) return; /* reference: loops do not execute */
    const int w_cell = (int)ceilf(width / (float)n_cols);
    const int h_cell = (int)ceilf(height / (float)n_rows);
    int cap_cell = (w_cell + 6) * (h_cell + 6);
    int32_t *tx = (int32_t *)malloc(sizeof(int32_t) * (size_t)cap_cell);
    int32_t *ty = (int32_t *)malloc(sizeof(int32_t) * (size_t)cap_cell);
    int32_t *ts = (int32_t *)malloc(sizeof(int32_t) * (size_t)cap_cell);
    const uint8_t *img = ex->pyr[level];
    for (int i = 0; i < n_rows; i++) {
        const float ini_y = (float)(min_by + i * h_cell);
        float max_y = ini_y + (float)h_cell + 6;
        if (ini_y >= (float)(max_by - 3)) continue;
        if (max_y > (float)max_by) max_y = (float)max_by;
        for (int j = 0; j < n_cols; j++) {
            const float ini_x = (float)(min_bx + j * w_cell);
            float max_x = ini_x + (float)w_cell + 6;
            if (ini_x >= (float)(max_bx - 6)) continue;
            if (max_x > (float)max_bx) max_x = (float)max_bx;
            int y0 = (int)ini_y, y1 = (int)max_y, x0 = (int)ini_x, x1 = (int)max_x;
            const uint8_t *cell = img + (size_t)y0 * lw + x0;
            int n = orc_fast9_16(cell, x1 - x0, y1 - y0, (size_t)lw, ex->p.ini_th_fast, 1, tx, ty, ts, cap_cell);
            if (n == 0)
                n = orc_fast9_16(cell, x1 - x0, y1 - y0, (size_t)lw, ex->p.min_th_fast, 1, tx, ty, ts, cap_cell);
            for (int k = 0; k < n; k++)
                cand_push(ex, level, &capc, tx[k] + j * w_cell, ty[k] + i * h_cell, ts[k]);
        }
    }
    free(tx); free(ty); free(ts);
}

/* ORBextractor::operator(), reference src/ORBextractor.cc:858-919 */
int orc_extract(orc_extractor *ex, const uint8_t *img, int w, int h, size_t stride,
                orc_keypoint *kps, uint8_t *desc, int cap)
{
    if (!ex) return -1;
    if (!img || w <= 0 || h <= 0) return 0; /* _image.empty(): silent return */
    free_state(ex);
    compute_pyramid(ex, img, w, h, stride);
    const int et = ex->p.edge_threshold;
    int total = 0;
    for (int level = 0; level < ex->p.nlevels; ++level) {
        level_candidates(ex, level);
        const int lw = ex->lw[level], lh = ex->lh[level];
        const int min_bx = et - 3, min_by = min_bx, max_bx = lw - et + 3, max_by = lh - et + 3;
        int nc = ex->ncand[level];
        int capk = ex->feats[level] + 16 + 4 * 64;
        int32_t *sel = (int32_t *)malloc(sizeof(int32_t) * (size_t)capk);
        int nk = 0;
        if (nc > 0 || 1) {
            nk = (max_bx > min_bx && max_by > min_by)
                     ? orc_distribute_octtree(ex->cx[level], ex->cy[level], ex->cs[level], nc, min_bx, max_bx,
                                              min_by, max_by, ex->feats[level], sel, capk)
                     : 0;
        }
        if (nk > capk) nk = capk;
        if (nk > 0) {
            /* src/ORBextractor.cc:899-900: blur a clone of the level */
            uint8_t *blur = (uint8_t *)malloc((size_t)lw * (size_t)lh);
            orc_gaussian7_u8(ex->pyr[level], lw, lh, (size_t)lw, blur, (size_t)lw);
            const int scaled_patch = (int)((float)ex->p.patch_size * ex->scale[level]);
            const float scale = ex->scale[level];
            for (int i = 0; i < nk; i++) {
                int c = sel[i];
                float px = (float)ex->cx[level][c] + (float)min_bx;
                float py = (float)ex->cy[level][c] + (float)min_by;
                int icx = orc_cv_round_f(px), icy = orc_cv_round_f(py);
                float ang = orc_ic_angle(ex->pyr[level], (size_t)lw, icx, icy, ex->umax, ex->p.half_patch_size);
                if (total < cap) {
                    orc_keypoint *kp = &kps[total];
                    orc_orb_descriptor_pat(blur, (size_t)lw, icx, icy, ang, ex->pattern, desc + (size_t)total * 32);
                    kp->x = px; kp->y = py;
                    if (level != 0) { kp->x = px * scale; kp->y = py * scale; }
                    kp->size = (float)scaled_patch;
                    kp->angle = ang;
                    kp->response = (float)ex->cs[level][c];
                    kp->octave = level;
                    kp->class_id = -1;
                }
                total++;
            }
            free(blur);
        }
        free(sel);
    }
    return total;
}

/* ------------------------------------------------------------------ */
/* Frame::ComputeStereoMatches, reference src/Frame.cc:464-642         */
/* ------------------------------------------------------------------ */

typedef struct dist_idx { int dist; int idx; } dist_idx;
static int cmp_dist_idx(const void *a, const void *b)
{
    const dist_idx *p = (const dist_idx *)a, *q = (const dist_idx *)b;
    if (p->dist != q->dist) return p->dist < q->dist ? -1 : 1;
    if (p->idx != q->idx) return p->idx < q->idx ? -1 : 1;
    return 0;
}

int orc_stereo_matches(const orc_extractor *exL, const orc_extractor *exR,
                       const orc_keypoint *kL, const uint8_t *dL, int nL,
                       const orc_keypoint *kR, const uint8_t *dR, int nR,
                       float bf, float fx, float *u_right, float *depth,
                       int32_t *best_idx_r, int32_t *best_sad)
{
    const int TH_HIGH = 100, TH_LOW = 50;
    for (int i = 0; i < nL; i++) {
        u_right[i] = -1.0f; depth[i] = -1.0f;
        if (best_idx_r) best_idx_r[i] = -1;
        if (best_sad) best_sad[i] = -1;
    }
    const int th_orb_dist = (TH_HIGH + TH_LOW) / 2;
    const int n_rows = exL->lh[0];
    if (n_rows <= 0) return 0;

    /* row table, :474-491 */
    int *row_cnt = (int *)calloc((size_t)n_rows + 1, sizeof(int));
    for (int iR = 0; iR < nR; iR++) {
        const float kp_y = kR[iR].y;
        const float r = 2.0f * exL->scale[kR[iR].octave];
        const int maxr = (int)ceilf(kp_y + r);
        const int minr = (int)floorf(kp_y - r);
        for (int yi = minr; yi <= maxr; yi++) if (yi >= 0 && yi < n_rows) row_cnt[yi + 1]++;
    }
    for (int i = 0; i < n_rows; i++) row_cnt[i + 1] += row_cnt[i];
    int *row_fill = (int *)malloc(sizeof(int) * (size_t)n_rows);
    memcpy(row_fill, row_cnt, sizeof(int) * (size_t)n_rows);
    int *row_idx = (int *)malloc(sizeof(int) * (size_t)(row_cnt[n_rows] > 0 ? row_cnt[n_rows] : 1));
    for (int iR = 0; iR < nR; iR++) {
        const float kp_y = kR[iR].y;
        const float r = 2.0f * exL->scale[kR[iR].octave];
        const int maxr = (int)ceilf(kp_y + r);
        const int minr = (int)floorf(kp_y - r);
        for (int yi = minr; yi <= maxr; yi++) if (yi >= 0 && yi < n_rows) row_idx[row_fill[yi]++] = iR;
    }

    /* Q1: mb := mbf/fx */
    const float mb = bf / fx;
    int nmatched = 0;
    dist_idx *vdi = (dist_idx *)malloc(sizeof(dist_idx) * (size_t)(nL > 0 ? nL : 1));
    int nvdi = 0;
    if (mb != 0) {
        const float min_z = mb;
        const float min_d = 0;
        const float max_d = bf / min_z;
        for (int iL = 0; iL < nL; iL++) {
            const orc_keypoint *kpL = &kL[iL];
            const int level_l = kpL->octave;
            const float vL = kpL->y, uL = kpL->x;
            int row = (int)vL;
            if (row < 0 || row >= n_rows) continue;
            const int *cand = row_idx + row_cnt[row];
            const int ncand = row_cnt[row + 1] - row_cnt[row];
            if (ncand == 0) continue;
            const float min_u = uL - max_d;
            const float max_u = uL - min_d;
            if (max_u < 0) continue;
            int best_dist = TH_HIGH;
            int best_r = 0;
            const uint8_t *dl = dL + (size_t)iL * 32;
            for (int ic = 0; ic < ncand; ic++) {
                const int iR = cand[ic];
                const orc_keypoint *kpR = &kR[iR];
                if (kpR->octave < level_l - 1 || kpR->octave > level_l + 1) continue;
                const float uR = kpR->x;
                if (uR >= min_u && uR <= max_u) {
                    const int dist = orc_hamming256(dl, dR + (size_t)iR * 32);
                    if (dist < best_dist) { best_dist = dist; best_r = iR; }
                }
            }
            if (best_dist < th_orb_dist) {
                if (best_idx_r) best_idx_r[iL] = best_r;
                const float uR0 = kR[best_r].x;
                const float sf = exL->inv_scale[kpL->octave];
                const float scaled_uL = roundf(kpL->x * sf);
                const float scaled_vL = roundf(kpL->y * sf);
                const float scaled_uR0 = roundf(uR0 * sf);
                const int w = 5, L = 5;
                const int lvl = kpL->octave;
                const uint8_t *imL = exL->pyr[lvl];
                const uint8_t *imR = exR->pyr[lvl];
                const int lwL = exL->lw[lvl], lwR = exR->lw[lvl];
                const int cu = (int)scaled_uL, cv = (int)scaled_vL, cr = (int)scaled_uR0;
                const float iniu = scaled_uR0 + (float)L - (float)w;
                const float endu = scaled_uR0 + (float)L + (float)w + 1;
                if (iniu < 0 || endu >= (float)exR->lw[lvl]) continue;
                /* Q12: the reference's guard is short by 2 w on the left (iniu = scaleduR0 + L - w = scaleduR0 is never negative): a right
                 * band that starts left of the level image (cr - 10 < 0) makes Mat::colRange throw cv::Exception (src/Frame.cc:582,
                 * CV_Assert(0 <= _colRange.start) in the cv::Mat ROI constructor) and the process ends.  Only reachable when
                 * 19 / scaleFactor < 10 (a right keypoint one octave finer than the left one, scaleFactor > 1.9); with the reference's
                 * 1.2 every window is inside.  Contract: such a keypoint stays unmatched (the product's memory-safety guard). */
                if (cu - 5 < 0 || cu + 5 >= lwL || cv - 5 < 0 || cv + 5 >= exL->lh[lvl] || cr - 10 < 0 || cr + 10 >= lwR) continue;
                int sad_best = INT_MAX, best_inc = 0;
                float vdists[11];
                const int lc = imL[(size_t)cv * lwL + cu];
                for (int inc = -L; inc <= L; inc++) {
                    const int rc = imR[(size_t)cv * lwR + cr + inc];
                    double acc = 0.0; /* cv::norm L1 on CV_32F accumulates in double (A.7) */
                    for (int dy = -w; dy <= w; dy++)
                        for (int dx = -w; dx <= w; dx++) {
                            float a = (float)imL[(size_t)(cv + dy) * lwL + cu + dx] - (float)lc;
                            float b = (float)imR[(size_t)(cv + dy) * lwR + cr + inc + dx] - (float)rc;
                            acc += (double)fabsf(a - b);
                        }
                    float dist = (float)acc;
                    if (dist < (float)sad_best) { sad_best = (int)dist; best_inc = inc; }
                    vdists[L + inc] = dist;
                }
                if (best_sad) best_sad[iL] = sad_best;
                if (best_inc == -L || best_inc == L) continue;
                const float dist1 = vdists[L + best_inc - 1];
                const float dist2 = vdists[L + best_inc];
                const float dist3 = vdists[L + best_inc + 1];
                const float delta_r = (dist1 - dist3) / (2.0f * (dist1 + dist3 - 2.0f * dist2));
                if (delta_r < -1 || delta_r > 1) continue;
                float best_ur = exL->scale[kpL->octave] * ((float)scaled_uR0 + (float)best_inc + delta_r);
                float disparity = (uL - best_ur);
                if (disparity >= min_d && disparity < max_d) {
                    if (disparity <= 0) {
                        disparity = (float)0.01;
                        best_ur = (float)((double)uL - 0.01);
                    }
                    depth[iL] = bf / disparity;
                    u_right[iL] = best_ur;
                    vdi[nvdi].dist = sad_best; vdi[nvdi].idx = iL; nvdi++;
                    nmatched++;
                }
            }
        }
        /* :628-641; Q2: skip when empty */
        if (nvdi > 0) {
            qsort(vdi, (size_t)nvdi, sizeof(dist_idx), cmp_dist_idx);
            const float median = (float)vdi[nvdi / 2].dist;
            const float th_dist = 1.5f * 1.4f * median;
            for (int i = nvdi - 1; i >= 0; i--) {
                if ((float)vdi[i].dist < th_dist) break;
                u_right[vdi[i].idx] = -1;
                depth[vdi[i].idx] = -1;
                nmatched--;
            }
        }
    }
    free(vdi); free(row_cnt); free(row_fill); free(row_idx);
    return nmatched;
}

/* Frame::ComputeStereoFromRGBD, reference src/Frame.cc:645-666 */
void orc_stereo_from_rgbd(const orc_keypoint *k, const orc_keypoint *k_un, int n,
                          const float *depth, int w, int h, size_t stride_floats,
                          float bf, float *u_right, float *out_depth)
{
    for (int i = 0; i < n; i++) {
        u_right[i] = -1; out_depth[i] = -1;
        int v = (int)k[i].y, u = (int)k[i].x;
        if (u < 0 || v < 0 || u >= w || v >= h) continue; /* guard: reference would read out of range */
        const float d = depth[(size_t)v * stride_floats + u];
        if (d > 0) {
            out_depth[i] = d;
            u_right[i] = k_un[i].x - bf / d;
        }
    }
}


/* cv::cvtColor(src, dst, COLOR_{RGB,BGR,RGBA,BGRA}2GRAY) for CV_8U, as Tracking::GrabImage{Monocular,Stereo,RGBD} call it
 * (src/Tracking.cc:269-294,305-321,335-351).  OPENCV-4.5.5-SEMANTICS: color_rgb.simd.hpp RGB2Gray<uchar> --
 * gray = (R*RY15 + G*GY15 + B*BY15 + (1 << 14)) >> 15 with RY15 = 9798, GY15 = 19235, BY15 = 3735 (sum 32768; alpha
 * ignored; the SIMD and scalar paths are bit-identical by construction).  OpenCV 3.x used 14-bit weights 4899 / 9617 / 1868
 * (sum 16384): `legacy14` selects those, so a build against an older OpenCV can be matched -- a configurable constant like
 * the Gaussian taps.  cn = 3 or 4; rgb != 0: channel 0 is red (mbRGB), else blue. */
void orc_cvt_gray(const uint8_t *src, int w, int h, size_t stride, int cn, int rgb, int legacy14, uint8_t *dst, size_t dst_stride)
{
    const int cr = legacy14 ? 4899 : 9798, cg = legacy14 ? 9617 : 19235, cb = legacy14 ? 1868 : 3735, shift = legacy14 ? 14 : 15;
    for (int y = 0; y < h; y++) {
        const uint8_t *s = src + (size_t)y * stride;
        uint8_t *d = dst + (size_t)y * dst_stride;
        for (int x = 0; x < w; x++, s += cn) {
            const int r = rgb ? s[0] : s[2], g = s[1], b = rgb ? s[2] : s[0];
            d[x] = (uint8_t)((unsigned)(r * cr + g * cg + b * cb + (1 << (shift - 1))) >> shift);
        }
    }
}


/* cv::undistortPoints(src, dst, K, D, cv::Mat(), K) as Frame::UndistortKeyPoints / ComputeImageBounds call it
 * (src/Frame.cc:402-462).  OPENCV-4.5.5-SEMANTICS: calib3d/undistort.dispatch.cpp cvUndistortPointsInternal with the
 * 6-argument overload's TermCriteria(MAX_ITER, 5, 0.01): exactly five fixed-point iterations in double, no error test;
 * K and D are CV_32F there and are widened to double; R = I, P = K so the re-projection is fx*x + 0*y + cx (w = 1).
 * dist = k1 k2 p1 p2 [k3] (ndist = 4 or 5, src/Tracking.cc:67-77).  The caller skips the call when k1 == 0 (:404-408). */
void orc_undistort_points(const float *src_xy, int n, float fx, float fy, float cx, float cy, const float *dist, int ndist, float *dst_xy)
{
    double k[14] = {0};
    for (int i = 0; i < ndist && i < 14; i++) k[i] = dist[i];
    const double dfx = fx, dfy = fy, dcx = cx, dcy = cy, ifx = 1. / dfx, ify = 1. / dfy;
    for (int i = 0; i < n; i++) {
        const double u = src_xy[2 * i], v = src_xy[2 * i + 1];
        double x = (u - dcx) * ifx, y = (v - dcy) * ify;
        const double x0 = x, y0 = y; /* tilt model absent (k[12] = k[13] = 0): invMatTilt is the identity */
        for (int j = 0; j < 5; j++) {
            const double r2 = x * x + y * y;
            const double icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);
            if (icdist < 0) { x = (u - dcx) * ifx; y = (v - dcy) * ify; break; }
            const double deltaX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2;
            const double deltaY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2;
            x = (x0 - deltaX) * icdist;
            y = (y0 - deltaY) * icdist;
        }
        const double xx = dfx * x + 0.0 * y + dcx, yy = 0.0 * x + dfy * y + dcy, ww = 1. / (0.0 * x + 0.0 * y + 1.0);
        dst_xy[2 * i] = (float)(xx * ww);
        dst_xy[2 * i + 1] = (float)(yy * ww);
    }
}

/* Frame::ComputeImageBounds (src/Frame.cc:434-462): bounds[4] = mnMinX, mnMaxX, mnMinY, mnMaxY */
void orc_image_bounds(int cols, int rows, float fx, float fy, float cx, float cy, const float *dist, int ndist, float *bounds)
{
    if (ndist > 0 && dist[0] != 0.0f) {
        const float c[8] = {0.f, 0.f, (float)cols, 0.f, 0.f, (float)rows, (float)cols, (float)rows};
        float o[8];
        orc_undistort_points(c, 4, fx, fy, cx, cy, dist, ndist, o);
        bounds[0] = o[0] < o[4] ? o[0] : o[4];  /* min(mat(0,0), mat(2,0)) */
        bounds[1] = o[2] > o[6] ? o[2] : o[6];  /* max(mat(1,0), mat(3,0)) */
        bounds[2] = o[1] < o[3] ? o[1] : o[3];  /* min(mat(0,1), mat(1,1)) */
        bounds[3] = o[5] > o[7] ? o[5] : o[7];  /* max(mat(2,1), mat(3,1)) */
    } else {
        bounds[0] = 0.f; bounds[1] = (float)cols; bounds[2] = 0.f; bounds[3] = (float)rows;
    }
}


/* cv::remap(src, dst, map1, map2, INTER_LINEAR) for CV_8UC1 with CV_32FC1 maps and the default BORDER_CONSTANT / Scalar()
 * (EuRoC rectification, Test/Replay/Stereo/stereo_euroc.cc:136-137, maps from initUndistortRectifyMap :98-99).
 * OPENCV-4.5.5-SEMANTICS (imgproc/src/imgwarp.cpp RemapInvoker + remapBilinear<FixedPtCast<int, uchar, 15>>): the float
 * maps become fixed point with 5 fraction bits, sx = cvRound(mapx * 32) (integer part saturated to short); the four taps
 * are weighted with BilinearTab_i = {(32-fx)(32-fy), fx(32-fy), (32-fx)fy, fx*fy} * 32 (exact integers, sum 2^15, so the
 * table's sum-correction step never fires) and the result is (sum + 2^14) >> 15.  A tap outside the source reads 0; a
 * destination pixel whose whole 2x2 footprint is outside is 0. */
static short sat_short(int v) { return (short)(v < -32768 ? -32768 : v > 32767 ? 32767 : v); }

void orc_remap_fixed(const float *mapx, const float *mapy, int n, int16_t *sx, int16_t *sy, uint16_t *alpha)
{
    for (int i = 0; i < n; i++) {
        const int ix = orc_cv_round_f(mapx[i] * 32.0f), iy = orc_cv_round_f(mapy[i] * 32.0f);
        sx[i] = sat_short(ix >> 5);
        sy[i] = sat_short(iy >> 5);
        alpha[i] = (uint16_t)((iy & 31) * 32 + (ix & 31));
    }
}

void orc_remap_bilinear(const uint8_t *src, int sw, int sh, size_t sstride, const float *mapx, const float *mapy,
                        int dw, int dh, uint8_t *dst, size_t dstride)
{
    for (int y = 0; y < dh; y++)
        for (int x = 0; x < dw; x++) {
            int16_t sx, sy; uint16_t a;
            orc_remap_fixed(mapx + (size_t)y * dw + x, mapy + (size_t)y * dw + x, 1, &sx, &sy, &a);
            const int fx = a & 31, fy = a >> 5;
            const int w[4] = {(32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32, (32 - fx) * fy * 32, fx * fy * 32};
            int v[4];
            for (int k = 0; k < 4; k++) {
                const int xx = sx + (k & 1), yy = sy + (k >> 1);
                v[k] = (xx >= 0 && xx < sw && yy >= 0 && yy < sh) ? src[(size_t)yy * sstride + xx] : 0;
            }
            dst[(size_t)y * dstride + x] = (uint8_t)((v[0] * w[0] + v[1] * w[1] + v[2] * w[2] + v[3] * w[3] + (1 << 14)) >> 15);
        }
}
