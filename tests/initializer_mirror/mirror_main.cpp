// mirror_main.cpp -- TEST-ONLY driver of orbslam2_amd/host/Initializer.h: reads the problem file that tests/initializer_scenes.py writes,
// runs ORB_SLAM2::NormalizeKeys on both frames and ORB_SLAM2::FindHomographyFundamental, and writes the outputs back.
// tests/test_initializer_model.py builds it twice with g++, plain and with -fsanitize=address,undefined.
//   file:  int32 n1, n2, N, iterations, norms_given;  float sigma, norm1[4], norm2[4] (used when norms_given);  x1[n1] y1[n1] x2[n2] y2[n2] (f32);  pairs[2 N] sets[8 iterations] (i32)
//   out:   int32 rc;  norm1[4] norm2[4] (NormalizeKeys of both frames);  H21[9] F21[9] score[2] (f32) best[2] (i32) inliers_h[N] inliers_f[N] (u8) ninliers[2] (i32)
//          all_scores[2 iterations] (f32) -- every output starts as a sentinel (-555, -7, 0xEE)
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
    std::vector<orbfe_keypoint> k(n);
    if (n) memset(k.data(), 0, n * sizeof(orbfe_keypoint));
    for (int i = 0; i < n; i++) { k[i].x = x[i]; k[i].y = y[i]; }
    return k;
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: %s problem.bin out.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const std::vector<int32_t> h = take<int32_t>(f, 5);
    const int n1 = h[0], n2 = h[1], N = h[2], iterations = h[3];
    const float sigma = take<float>(f, 1)[0];
    const auto given = take<float>(f, 8);
    const auto keys1 = read_keys(f, n1), keys2 = read_keys(f, n2);
    const auto pairs = take<int32_t>(f, 2 * (size_t)N), sets = take<int32_t>(f, 8 * (size_t)iterations);
    fclose(f);

    std::vector<float> norms(8), H21(9, -555.f), F21(9, -555.f), score(2, -555.f), all_scores(2 * (size_t)iterations, -555.f);
    std::vector<int32_t> best(2, -7), ninliers(2, -7);
    std::vector<uint8_t> inl_h(N, 0xEE), inl_f(N, 0xEE);
    ORB_SLAM2::NormalizeKeys(keys1.data(), n1, norms.data());
    ORB_SLAM2::NormalizeKeys(keys2.data(), n2, norms.data() + 4);
    // a vector of size 0 has no storage to point at: empty arrays get a dummy cell that is never read or written
    uint8_t no_flag = 0; int32_t no_index = 0; float no_score = 0;
    const int32_t rc = ORB_SLAM2::FindHomographyFundamental(keys1.data(), n1, keys2.data(), n2, N ? pairs.data() : &no_index, N, iterations ? sets.data() : &no_index,
                                                            iterations, h[4] ? given.data() : norms.data(), h[4] ? given.data() + 4 : norms.data() + 4, sigma, H21.data(), F21.data(), score.data(), best.data(),
                                                            N ? inl_h.data() : &no_flag, N ? inl_f.data() : &no_flag, ninliers.data(),
                                                            iterations ? all_scores.data() : &no_score);
    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    put(o, std::vector<int32_t>{rc});
    put(o, norms); put(o, H21); put(o, F21); put(o, score); put(o, best); put(o, inl_h); put(o, inl_f); put(o, ninliers); put(o, all_scores);
    fclose(o);
    return 0;
}
