// mirror_main.cpp -- TEST-ONLY driver of ORB_SLAM2::ReconstructInitial (orbslam2_amd/host/Initializer.h): reads the problem file that
// tests/reconstruct_scenes.py writes, runs the call and writes the outputs back.  tests/test_reconstruct_model.py builds it twice with
// g++, plain and with -fsanitize=address,undefined.
//   file:  int32 n1, n2, N, min_triangulated, model;  float sigma, K[4], H21[9], F21[9], score[2];  int32 best[2];
//          x1[n1] y1[n1] x2[n2] y2[n2] (f32);  pairs[2 N] (i32);  inliers_h[N] inliers_f[N] (u8)
//   out:   int32 rc;  model[1] (i32) hyp_R[72] hyp_t[24] (f32) ngood[8] (i32) cos_parallax[8] (f32) result[1] choice[1] (i32) R21[9] t21[3]
//          p3d[3 n1] (f32) triangulated[n1] codes[8 N] (u8) -- every output starts as a sentinel (-555, -7, 0xEE)
//   with a third argument "accept": prints ReconstructAccept(model, cos, min_parallax) for the three numbers that follow
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../orbslam2_amd/host/Initializer.h"

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

static std::vector<orbfe_keypoint> read_keys(FILE *f, int n)
{
    const auto x = take<float>(f, n), y = take<float>(f, n);
    std::vector<orbfe_keypoint> k(n + 1); // never empty: the call wants a pointer
    memset(k.data(), 0, k.size() * sizeof(orbfe_keypoint));
    for (int i = 0; i < n; i++) { k[i].x = x[i]; k[i].y = y[i]; }
    return k;
}

int main(int argc, char **argv)
{
    if (argc == 5 && !strcmp(argv[1], "accept")) {
        printf("%d\n", (int)ORB_SLAM2::ReconstructAccept(atoi(argv[2]), strtof(argv[3], nullptr), strtof(argv[4], nullptr)));
        return 0;
    }
    if (argc < 3) { fprintf(stderr, "usage: %s problem.bin out.bin | accept model cos min_parallax\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const std::vector<int32_t> h = take<int32_t>(f, 5);
    const int n1 = h[0], n2 = h[1], N = h[2], min_triangulated = h[3], model = h[4];
    const float sigma = take<float>(f, 1)[0];
    const auto K = take<float>(f, 4), H21 = take<float>(f, 9), F21 = take<float>(f, 9), score = take<float>(f, 2);
    const auto best = take<int32_t>(f, 2);
    const auto keys1 = read_keys(f, n1), keys2 = read_keys(f, n2);
    const size_t n = N > 0 ? (size_t)N : 0;
    auto pairs = take<int32_t>(f, 2 * n);
    auto inl_h = take<uint8_t>(f, n), inl_f = take<uint8_t>(f, n);
    fclose(f);

    std::vector<int32_t> out_model(1, -7), ngood(8, -7), result(1, -7), choice(1, -7);
    std::vector<float> hyp_R(72, -555.f), hyp_t(24, -555.f), cosp(8, -555.f), R21(9, -555.f), t21(3, -555.f), p3d(3 * (size_t)n1, -555.f);
    std::vector<uint8_t> tri(n1, 0xEE), codes(8 * n, 0xEE);
    // a vector of size 0 has no storage to point at: empty arrays get a dummy cell that is never read or written
    int32_t no_index[2] = {0, 0}; uint8_t no_flag = 0; float no_point[3] = {0, 0, 0};
    const int32_t rc = ORB_SLAM2::ReconstructInitial(keys1.data(), n1, keys2.data(), n2, n ? pairs.data() : no_index, N, H21.data(), F21.data(), score.data(), best.data(),
                                                     n ? inl_h.data() : &no_flag, n ? inl_f.data() : &no_flag, K.data(), sigma, min_triangulated, model, out_model.data(),
                                                     hyp_R.data(), hyp_t.data(), ngood.data(), cosp.data(), result.data(), choice.data(), R21.data(), t21.data(),
                                                     n1 ? p3d.data() : no_point, n1 ? tri.data() : &no_flag, n ? codes.data() : &no_flag);
    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    put(o, std::vector<int32_t>{rc});
    put(o, out_model); put(o, hyp_R); put(o, hyp_t); put(o, ngood); put(o, cosp); put(o, result); put(o, choice); put(o, R21); put(o, t21);
    put(o, p3d); put(o, tri); put(o, codes);
    fclose(o);
    return 0;
}
