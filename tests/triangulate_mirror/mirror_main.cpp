// mirror_main.cpp -- TEST-ONLY driver of orbslam2_amd/host/Triangulate.h: reads the problem file that tests/triangulate_scenes.py writes,
// runs ORB_SLAM2::TriangulatePairs on it and writes the outputs back.  tests/test_triangulate_model.py builds it twice with g++, plain
// and with -fsanitize=address,undefined.
//   file:  int32 n1, n2, npairs, max_pairs, nlevels, has_pos, n_rows, rows_used, patch;  float mbf, ratio
//          per keyframe: Tcw[12] Ow[3] fx fy cx cy invfx invfy (f32), x_un[n] y_un[n] (f32) octave[n] (i32) x[n] y[n] ur[n] depth[n] cos[n] (f32) mp[n] (u8)
//          pairs[2 * max_pairs] (i32)  scale[nlevels] sigma2[nlevels] (f32)  code[max_pairs] (u8) x3d[3 * max_pairs] (f32) new[3 * max_pairs] (i32)
//          pos[3 * n_rows] (f32) if has_pos
//   out:   int32 status, nnew (-7: untouched), rows_used; code, x3d, new, pos if has_pos, mp1, mp2
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../orbslam2_amd/host/Triangulate.h"

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

struct Keyframe {
    std::vector<orbfe_keypoint> keys_un, keys;
    std::vector<float> ur, depth, cos_stereo;
    std::vector<uint8_t> mp;
    orbfe_newpoint_keyframe rec;
};

static void read_keyframe(FILE *f, int n, Keyframe &k)
{
    const auto head = take<float>(f, 21);
    const auto xu = take<float>(f, n), yu = take<float>(f, n);
    const auto octave = take<int32_t>(f, n);
    const auto x = take<float>(f, n), y = take<float>(f, n);
    k.ur = take<float>(f, n); k.depth = take<float>(f, n); k.cos_stereo = take<float>(f, n);
    k.mp = take<uint8_t>(f, n);
    k.keys_un.resize(n); k.keys.resize(n);
    if (n) { memset(k.keys_un.data(), 0, n * sizeof(orbfe_keypoint)); memset(k.keys.data(), 0, n * sizeof(orbfe_keypoint)); }
    for (int i = 0; i < n; i++) {
        k.keys_un[i].x = xu[i]; k.keys_un[i].y = yu[i]; k.keys_un[i].octave = octave[i];
        k.keys[i].x = x[i]; k.keys[i].y = y[i]; k.keys[i].octave = octave[i];
    }
    orbfe_newpoint_keyframe &r = k.rec;
    r.keys_un = k.keys_un.data(); r.keys = k.keys.data(); r.u_right = k.ur.data(); r.depth = k.depth.data(); r.cos_stereo = k.cos_stereo.data();
    r.has_mp = k.mp.data();
    for (int c = 0; c < 12; c++) r.Tcw[c] = head[c];
    for (int c = 0; c < 3; c++) r.Ow[c] = head[12 + c];
    r.fx = head[15]; r.fy = head[16]; r.cx = head[17]; r.cy = head[18]; r.invfx = head[19]; r.invfy = head[20];
    r.n = n;
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: %s problem.bin out.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const std::vector<int32_t> h = take<int32_t>(f, 9);
    const int n1 = h[0], n2 = h[1], max_pairs = h[3], nlevels = h[4], has_pos = h[5], n_rows = h[6], patch = h[8];
    const int32_t npairs = h[2];
    const auto fl = take<float>(f, 2);
    Keyframe k1, k2;
    read_keyframe(f, n1, k1);
    read_keyframe(f, n2, k2);
    const auto pairs = take<int32_t>(f, 2 * (size_t)max_pairs);
    const auto scale = take<float>(f, nlevels), sigma2 = take<float>(f, nlevels);
    auto code = take<uint8_t>(f, max_pairs);
    auto x3d = take<float>(f, 3 * (size_t)max_pairs);
    auto new_points = take<int32_t>(f, 3 * (size_t)max_pairs);
    auto pos = take<float>(f, has_pos ? 3 * (size_t)n_rows : 0);
    fclose(f);
    // a vector of size 0 has no storage to point at: the call refuses NULL outputs, so empty ones get a dummy cell that is never written
    uint8_t no_code = 0; float no_x = 0; int32_t no_new = 0, no_pair = 0;

    int32_t nnew = -7, rows_used = h[7];
    const int32_t status = ORB_SLAM2::TriangulatePairs(&k1.rec, &k2.rec, fl[0], fl[1], max_pairs ? pairs.data() : &no_pair, &npairs, max_pairs, scale.data(),
                                                       sigma2.data(), nlevels, max_pairs ? code.data() : &no_code, max_pairs ? x3d.data() : &no_x,
                                                       max_pairs ? new_points.data() : &no_new, &nnew, has_pos ? (n_rows ? pos.data() : &no_x) : nullptr, n_rows,
                                                       has_pos ? &rows_used : nullptr, patch);
    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    put(o, std::vector<int32_t>{status, nnew, rows_used});
    put(o, code); put(o, x3d); put(o, new_points); put(o, pos); put(o, k1.mp); put(o, k2.mp);
    fclose(o);
    return 0;
}
