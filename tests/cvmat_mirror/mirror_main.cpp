// mirror_main.cpp -- TEST-ONLY driver of orbslam2_amd/host/CvMat.h: reads the problem file that tests/test_cvmat_model.py writes, runs the
// shared Jacobi on every matrix and the 3 x 3 steps on every pair of 3 x 3 inputs, and writes the outputs back.  Built twice with g++
// through tests/host_forms.py, plain and with -fsanitize=address,undefined.  The file holds the known-answer matrices and, after them, the
// seeded ones (seeded_jacobi_inputs, seeded_small_inputs: duplicated and zero columns, a NaN and an Inf entry, singular and nearly singular
// 3 x 3) that tests/test_arith_blocks.py gives the device forms: the counts in the file say how many, so the loops below run them all.
//   file:  int32 nj;  nj x { int32 n, m;  f32 A[m][n] };  int32 n3;  n3 x { f32 a[9], b[9], plus[9];  f64 alpha };  int32 ns;  f32 v[ns]
//   out:   nj x { f32 At[n][16], Vt[n][9];  f64 W[n];  int32 sweeps }
//          n3 x { f32 u[9], w[3], vt[9] (Svd3 of a), inv[9] (Inv3 of a), ab[9] (a * b), abp[9] (alpha * a * b + plus), unit[3] (Unit of a's
//                 row 0);  f64 det (Det3 of a), norm (Norm3 of a's row 0) }
//          f32 stored[ns]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../orbslam2_amd/host/CvMat.h"

template <class T> static std::vector<T> take(FILE *f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short problem file\n"); exit(2); }
    return v;
}

template <class T> static void put(FILE *f, const std::vector<T> &v)
{
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "short write\n"); exit(2); }
}

int main(int argc, char **argv)
{
    using namespace ORB_SLAM2;
    if (argc < 3) { fprintf(stderr, "usage: %s problem.bin out.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    const int nj = take<int32_t>(f, 1)[0];
    for (int q = 0; q < nj; q++) {
        const auto h = take<int32_t>(f, 2);
        const int n = h[0], m = h[1];
        if (n < 1 || n > kCvMatVStride || m < n || m > kCvMatAStride) { fprintf(stderr, "a %d x %d matrix does not fit\n", m, n); return 2; }
        const auto A = take<float>(f, (size_t)m * n);
        std::vector<float> At((size_t)n * kCvMatAStride, 0.f), Vt((size_t)n * kCvMatVStride, 0.f);
        std::vector<double> W(n);
        for (int i = 0; i < n; i++)
            for (int k = 0; k < m; k++) At[i * kCvMatAStride + k] = A[(size_t)k * n + i];
        const int32_t sweeps = Jacobi(At.data(), Vt.data(), W.data(), n, m);
        put(o, At); put(o, Vt); put(o, W); put(o, std::vector<int32_t>{sweeps});
    }
    const int n3 = take<int32_t>(f, 1)[0];
    for (int q = 0; q < n3; q++) {
        const auto a = take<float>(f, 9), b = take<float>(f, 9), plus = take<float>(f, 9);
        const double alpha = take<double>(f, 1)[0];
        std::vector<float> u(9), w(3), vt(9), inv(9), ab(9), abp(9), unit(a.begin(), a.begin() + 3);
        Svd3(a.data(), u.data(), w.data(), vt.data());
        Inv3(a.data(), inv.data());
        MatMul(a.data(), b.data(), 3, 3, 3, ab.data());
        MatMul(a.data(), b.data(), 3, 3, 3, abp.data(), &alpha, plus.data());
        Unit(unit.data());
        put(o, u); put(o, w); put(o, vt); put(o, inv); put(o, ab); put(o, abp); put(o, unit);
        put(o, std::vector<double>{Det3(a.data()), Norm3(a.data())});
    }
    auto v = take<float>(f, take<int32_t>(f, 1)[0]);
    for (float &x : v) x = Stored(x);
    put(o, v);
    fclose(f);
    fclose(o);
    return 0;
}
