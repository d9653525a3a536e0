// TEST-ONLY: runs the shared __device__ arithmetic of orbslam2_amd/csrc (orbfe_common.hpp, orbfe_cvmat.hpp, orbfe_jacobi4.hpp,
// orbfe_jacobi_wave.hpp) one helper at a time, so that tests/test_arith_blocks.py can compare raw bits with the oracle, the Python
// model and numpy.  Compiled with the product's flags; the headers are included as they are; nothing here is linked into liborbfe.so.
//
// arith_blocks_run(op, n, in, out): host arrays in, host arrays out.  Arrays of several inputs are planar (all y, then all x).
//   op                 n                in                                       out
//   ATAN2              pairs            f32 y[n], x[n]                           f32 [n]
//   SINCOS             arguments        f32 rad[n]                               f32 sin[n], cos[n]
//   SMALL_DIV          divisors         i32 b[n] (every a in [0, 2^21) is tried) u64 mismatches, first failing (a << 32 | b), ~0 if none
//   REFLECT101         pairs            i32 p[n], len[n]                         i32 [n]
//   ROW_SUM .. WAVE_MIN  vectors        u32 [n][64]                              u32 [n][64]: what every lane holds
//   SCAN               elements (>= 0)  i32 nt, alias, lds, src[n]               i32 total, dst[n]
//   DSQRT, D2F, D2I    values           f64 [n]                                  f64 / f32 / i32 [n]
//   DDIV               pairs            f64 a[n], b[n]                           f64 [n]
//   FDIV               pairs            f32 a[n], b[n]                           f32 [n]
//   SQRT_RN            values           f32 [n]                                  f32 [n]
//   MAT3               cases            Mat3In[n]                                Mat3Out[n]
//   JACOBI_3_4 / _9_16 matrices         f32 At[n][N][16]                         n x { f32 At[N][16], Vt[N][9], pad to 8 bytes; f64 W[N] }
//   NULL4              matrices         f32 At[n][4][4]                          n x { f32 v[4], Vt[4][4]; f64 W[4] }
// The Jacobi kernels have the product's launch shape: one 64-thread workgroup per matrix, At / Vt / W in LDS at AT_STRIDE / VT_STRIDE.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "orbfe_common.hpp"
#include "orbfe_cvmat.hpp"
#include "orbfe_jacobi4.hpp"
#include "orbfe_jacobi_wave.hpp"

namespace {

enum {
    OP_ATAN2 = 1, OP_SINCOS, OP_SMALL_DIV, OP_REFLECT101, OP_ROW_SUM, OP_WAVE_SUM, OP_WAVE_MIN_DPP, OP_WAVE_MIN, OP_SCAN, OP_DSQRT, OP_DDIV,
    OP_FDIV, OP_SQRT_RN, OP_D2F, OP_D2I, OP_MAT3, OP_JACOBI_3_4, OP_JACOBI_9_16, OP_NULL4, OP_END
};
constexpr int SMALL_DIV_A = 1 << 21, SMALL_DIV_CHUNKS = 32, SCAN_MAX_THREADS = 1024, SCAN_MAX_N = 5 * SCAN_MAX_THREADS + 3, MAX_N = 1 << 23;

struct Mat3In {
    float a[9], b[9], v[3], T[12], x[3], plus[3], pad;
    double alpha, nom, den;
};
struct Mat3Out {
    float ab[9], ab_alpha[9], inv[9], unit[3], stored[9], av[3], rwc_plus[3], rwc[3], row_dot[3], reduce, ratio;
    uint32_t fin[9], pad[2];
    double det, norm, dot, sum_sq;
};
static_assert(sizeof(Mat3In) == 184 && sizeof(Mat3Out) == 288, "the records tests/test_arith_blocks.py declares");

// ---------------------------------------------------------------------------------------------------------------- one element per thread
__global__ __launch_bounds__(256) void element_kernel(int op, int n, const void *__restrict__ in, void *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float *f = (const float *)in;
    const double *d = (const double *)in;
    const int *q = (const int *)in;
    switch (op) {
    case OP_ATAN2: ((float *)out)[i] = fast_atan2_deg(f[i], f[(size_t)n + i]); break;
    case OP_SINCOS: {
        float s, c;
        sincos_det(f[i], &s, &c);
        ((float *)out)[i] = s;
        ((float *)out)[(size_t)n + i] = c;
        break;
    }
    case OP_REFLECT101: ((int *)out)[i] = reflect101(q[i], q[(size_t)n + i]); break;
    case OP_DSQRT: ((double *)out)[i] = sqrt(d[i]); break;
    case OP_DDIV: ((double *)out)[i] = d[i] / d[(size_t)n + i]; break;
    case OP_FDIV: ((float *)out)[i] = __fdiv_rn(f[i], f[(size_t)n + i]); break;
    case OP_SQRT_RN: ((float *)out)[i] = sqrt_rn(f[i]); break;
    case OP_D2F: ((float *)out)[i] = (float)d[i]; break;
    case OP_D2I: ((int *)out)[i] = (int)d[i]; break;
    default: break;
    }
}

// every a of one chunk of [0, 2^21) against divisor b[blockIdx.y]: q * b <= a < (q + 1) * b in 64-bit integers
__global__ __launch_bounds__(256) void small_div_kernel(int n, const int *__restrict__ b_in, unsigned long long *__restrict__ out)
{
    if ((int)blockIdx.y >= n) return;
    const int b = b_in[blockIdx.y];
    constexpr int PER_BLOCK = SMALL_DIV_A / SMALL_DIV_CHUNKS;
    unsigned long long bad = 0, first = ~0ull;
    for (int a = blockIdx.x * PER_BLOCK + threadIdx.x; a < (int)(blockIdx.x + 1) * PER_BLOCK; a += 256) {
        const long long qq = small_div(a, b);
        if (!(qq * b <= (long long)a && (long long)a < (qq + 1) * b)) {
            bad++;
            const unsigned long long key = ((unsigned long long)(unsigned)a << 32) | (unsigned)b;
            first = key < first ? key : first;
        }
    }
    if (bad) {
        atomicAdd(&out[0], bad);
        atomicMin(&out[1], first);
    }
}

// one full wave per vector: all 64 lanes active, as the helpers require
__global__ __launch_bounds__(64) void wave_kernel(int op, int n, const uint32_t *__restrict__ in, uint32_t *__restrict__ out)
{
    if ((int)blockIdx.x >= n) return; // uniform
    const size_t at = (size_t)blockIdx.x * 64 + threadIdx.x;
    const uint32_t v = in[at];
    uint32_t r;
    if (op == OP_ROW_SUM) r = (uint32_t)row_sum_i32((int)v);
    else if (op == OP_WAVE_SUM) r = (uint32_t)wave_sum_i32((int)v);
    else if (op == OP_WAVE_MIN_DPP) r = wave_min_u32_dpp(v);
    else r = wave_min_u32(v);
    out[at] = r;
}

// block_excl_scan over n ints by blockDim.x threads; io = {nt, alias, lds, src[n]}; out = {total, dst[n]}
__global__ __launch_bounds__(SCAN_MAX_THREADS) void scan_kernel(int n, int alias, int lds, int *__restrict__ io, int *__restrict__ out)
{
    __shared__ int s_tmp[SCAN_MAX_THREADS], s_src[SCAN_MAX_N], s_dst[SCAN_MAX_N];
    int *g_src = io + 3, *g_dst = out + 1;
    int total;
    if (lds) {
        for (int i = threadIdx.x; i < n; i += blockDim.x) { s_src[i] = g_src[i]; s_dst[i] = 0; }
        __syncthreads();
        total = block_excl_scan(s_src, alias ? s_src : s_dst, n, s_tmp);
        const int *res = alias ? s_src : s_dst;
        for (int i = threadIdx.x; i < n; i += blockDim.x) g_dst[i] = res[i];
    } else {
        total = block_excl_scan(g_src, alias ? g_src : g_dst, n, s_tmp);
        if (alias) {
            __syncthreads();
            for (int i = threadIdx.x; i < n; i += blockDim.x) g_dst[i] = g_src[i];
        }
    }
    if (threadIdx.x == 0) out[0] = total;
}

// the 3 x 3 steps of orbfe_cvmat.hpp, one case per lane
__global__ __launch_bounds__(64) void mat3_kernel(int n, const Mat3In *__restrict__ in, Mat3Out *__restrict__ out)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const Mat3In c = in[i];
    Mat3Out o;
    mul3(c.a, c.b, o.ab);
    mul3_alpha(c.alpha, c.a, c.b, o.ab_alpha);
    inv3(c.a, o.inv);
    o.det = det3(c.a);
#pragma unroll
    for (int k = 0; k < 3; k++) o.unit[k] = c.v[k];
    unit3(o.unit);
    o.norm = norm3(c.v);
#pragma unroll
    for (int k = 0; k < 9; k++) {
        o.stored[k] = one_nan(c.a[k]);
        o.fin[k] = finite(c.a[k]) ? 1u : 0u;
    }
    mul3_vec(c.a, c.v, o.av);
    rwc_times(c.T, c.x, c.plus, o.rwc_plus);
    rwc_times(c.T, c.x, nullptr, o.rwc);
    o.row_dot[0] = row_dot_plus<0>(c.T, c.x);
    o.row_dot[1] = row_dot_plus<1>(c.T, c.x);
    o.row_dot[2] = row_dot_plus<2>(c.T, c.x);
    o.reduce = reduce_sum3(c.a[0], c.a[1], c.a[2]);
    o.ratio = ratio(c.nom, c.den);
    o.dot = dot9(c.a, c.b);
    o.sum_sq = sum_of_squared_floats9(c.a);
    o.pad[0] = o.pad[1] = 0u;
    out[i] = o;
}

constexpr size_t jacobi_out_bytes(int N) { return (((size_t)N * (AT_STRIDE + VT_STRIDE) + 1) & ~(size_t)1) * sizeof(float) + (size_t)N * sizeof(double); }

// jacobi_wave<N, M> as its callers launch it: one 64-thread workgroup per matrix, At / Vt / W in LDS
template <int N, int M>
__global__ __launch_bounds__(64) void jacobi_wave_kernel(int n, const float *__restrict__ in, uint8_t *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) float At[N * AT_STRIDE];
    __shared__ float Vt[N * VT_STRIDE];
    __shared__ double W[N];
    if ((int)blockIdx.x >= n) return; // uniform
    const int lane = threadIdx.x;
    const float *src = in + (size_t)blockIdx.x * N * AT_STRIDE;
    for (int k = lane; k < N * AT_STRIDE; k += 64) At[k] = src[k];
    for (int k = lane; k < N * VT_STRIDE; k += 64) Vt[k] = 0.f;
    if (lane < N) W[lane] = 0;
    __syncthreads();
    jacobi_wave<N, M>(At, Vt, W, lane);
    __syncthreads();
    uint8_t *rec = out + (size_t)blockIdx.x * jacobi_out_bytes(N);
    float *fo = (float *)rec;
    double *wo = (double *)(rec + jacobi_out_bytes(N) - (size_t)N * sizeof(double));
    for (int k = lane; k < N * AT_STRIDE; k += 64) fo[k] = At[k];
    for (int k = lane; k < N * VT_STRIDE; k += 64) fo[N * AT_STRIDE + k] = Vt[k];
    if (lane < N) wo[lane] = W[lane];
}

// null_vector of orbfe_jacobi4.hpp, one matrix per lane in registers
__global__ __launch_bounds__(64) void null4_kernel(int n, const float *__restrict__ in, uint8_t *__restrict__ out)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    Jacobi m;
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int k = 0; k < 4; k++) m.At[r][k] = in[(size_t)i * 16 + 4 * r + k];
    float v[4];
    null_vector(m, v);
    float *fo = (float *)(out + (size_t)i * 112);
    double *wo = (double *)(out + (size_t)i * 112 + 80);
#pragma unroll
    for (int k = 0; k < 4; k++) fo[k] = v[k];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int k = 0; k < 4; k++) fo[4 + 4 * r + k] = m.Vt[r][k];
#pragma unroll
    for (int k = 0; k < 4; k++) wo[k] = m.W[k];
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

// bytes of `in` and `out` per unit of n, and a fixed part
bool sizes(int op, int n, size_t &in_bytes, size_t &out_bytes)
{
    const size_t N = (size_t)n;
    switch (op) {
    case OP_ATAN2: in_bytes = 8 * N; out_bytes = 4 * N; return true;
    case OP_SINCOS: in_bytes = 4 * N; out_bytes = 8 * N; return true;
    case OP_SMALL_DIV: in_bytes = 4 * N; out_bytes = 16; return true;
    case OP_REFLECT101: in_bytes = 8 * N; out_bytes = 4 * N; return true;
    case OP_ROW_SUM: case OP_WAVE_SUM: case OP_WAVE_MIN_DPP: case OP_WAVE_MIN: in_bytes = out_bytes = 256 * N; return true;
    case OP_SCAN: in_bytes = 4 * (3 + N); out_bytes = 4 * (1 + N); return true;
    case OP_DSQRT: in_bytes = out_bytes = 8 * N; return true;
    case OP_DDIV: in_bytes = 16 * N; out_bytes = 8 * N; return true;
    case OP_FDIV: in_bytes = 8 * N; out_bytes = 4 * N; return true;
    case OP_SQRT_RN: in_bytes = out_bytes = 4 * N; return true;
    case OP_D2F: case OP_D2I: in_bytes = 8 * N; out_bytes = 4 * N; return true;
    case OP_MAT3: in_bytes = sizeof(Mat3In) * N; out_bytes = sizeof(Mat3Out) * N; return true;
    case OP_JACOBI_3_4: in_bytes = sizeof(float) * 3 * AT_STRIDE * N; out_bytes = jacobi_out_bytes(3) * N; return true;
    case OP_JACOBI_9_16: in_bytes = sizeof(float) * 9 * AT_STRIDE * N; out_bytes = jacobi_out_bytes(9) * N; return true;
    case OP_NULL4: in_bytes = 64 * N; out_bytes = 112 * N; return true;
    default: return false;
    }
}

} // namespace

// Host arrays in, host arrays out; 0 on success, -1 bad argument, -2 HIP error.
extern "C" int arith_blocks_run(int op, int n, const void *in, void *out)
{
    if (op < OP_ATAN2 || op >= OP_END || !in || !out || n > MAX_N) return -1;
    if (op == OP_SCAN ? (n < 0 || n > SCAN_MAX_N) : n <= 0) return -1;
    const bool per_wave = (op >= OP_ROW_SUM && op <= OP_WAVE_MIN) || op == OP_JACOBI_3_4 || op == OP_JACOBI_9_16;
    if ((per_wave && n > (1 << 20)) || (op == OP_SMALL_DIV && n > 65535)) return -1; // one workgroup each; grid y
    int nt = 0, alias = 0, lds = 0;
    if (op == OP_SCAN) {
        const int *h = (const int *)in;
        nt = h[0]; alias = h[1]; lds = h[2];
        if (nt < 1 || nt > SCAN_MAX_THREADS || (alias & ~1) || (lds & ~1)) return -1;
    }
    if (op == OP_SMALL_DIV)
        for (int i = 0; i < n; i++)
            if (((const int *)in)[i] < 1) return -1;
    size_t in_bytes, out_bytes;
    if (!sizes(op, n, in_bytes, out_bytes)) return -1;
    Dev d_in, d_out;
    if (!d_in.up(in, in_bytes) || !d_out.up(nullptr, out_bytes) || hipMemset(d_out.p, op == OP_SMALL_DIV ? 0xff : 0, out_bytes) != hipSuccess) return -2;
    if (op == OP_SMALL_DIV && hipMemset(d_out.p, 0, 8) != hipSuccess) return -2; // the count; the first failing pair stays ~0
    switch (op) {
    case OP_SMALL_DIV: hipLaunchKernelGGL(small_div_kernel, dim3(SMALL_DIV_CHUNKS, n), dim3(256), 0, 0, n, (const int *)d_in.p, (unsigned long long *)d_out.p); break;
    case OP_ROW_SUM: case OP_WAVE_SUM: case OP_WAVE_MIN_DPP: case OP_WAVE_MIN:
        hipLaunchKernelGGL(wave_kernel, dim3(n), dim3(64), 0, 0, op, n, (const uint32_t *)d_in.p, (uint32_t *)d_out.p);
        break;
    case OP_SCAN: hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(nt), 0, 0, n, alias, lds, (int *)d_in.p, (int *)d_out.p); break;
    case OP_MAT3: hipLaunchKernelGGL(mat3_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, n, (const Mat3In *)d_in.p, (Mat3Out *)d_out.p); break;
    case OP_JACOBI_3_4: hipLaunchKernelGGL((jacobi_wave_kernel<3, 4>), dim3(n), dim3(64), 0, 0, n, (const float *)d_in.p, (uint8_t *)d_out.p); break;
    case OP_JACOBI_9_16: hipLaunchKernelGGL((jacobi_wave_kernel<9, 16>), dim3(n), dim3(64), 0, 0, n, (const float *)d_in.p, (uint8_t *)d_out.p); break;
    case OP_NULL4: hipLaunchKernelGGL(null4_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, n, (const float *)d_in.p, (uint8_t *)d_out.p); break;
    default: hipLaunchKernelGGL(element_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, op, n, d_in.p, d_out.p); break;
    }
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -2;
    return hipMemcpy(out, d_out.p, out_bytes, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -2;
}
