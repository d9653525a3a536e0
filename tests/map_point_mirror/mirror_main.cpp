// mirror_main.cpp -- TEST-ONLY driver of orbslam2_amd/host/MapPointUpdate.h: reads the scene file that tests/map_point_scenes.py writes,
// runs ORB_SLAM2::UpdateMapPoints on it (or, with "bench K", K times and prints the best wall time) and writes the table back.
// tests/test_map_point_model.py builds it twice with g++, plain and with -fsanitize=address,undefined.
//   file:  int32 n_kfs, n_kp (all keyframes), n_upd, n_rows, n_obs, what, nlevels, has_row
//          kf_n[n_kfs] kf_bad[n_kfs] kf_first[n_kfs] (i32)  Ow[n_kfs][3] (f32)  desc[n_kp][32] (u8)  octave[n_kp] (i32)
//          row[n_upd] if has_row   obs_off[n_upd + 1]  obs_kf[n_obs]  obs_idx[n_obs]  ref[n_upd] (i32)  scale[nlevels] (f32)
//          pos[n_rows][3] normal[n_rows][3] max_d[n_rows] min_d[n_rows] (f32)  pt_desc[n_rows][32] (u8)
//   out:   int32 status, best[n_upd] (i32), normal, max_d, min_d (f32), pt_desc (u8)
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../orbslam2_amd/host/MapPointUpdate.h"

template <class T> static std::vector<T> take(FILE *f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short scene file\n"); exit(2); }
    return v;
}

template <class T> static void put(FILE *f, const std::vector<T> &v)
{
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "short write\n"); exit(2); }
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: %s scene.bin out.bin [bench K]\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const std::vector<int32_t> h = take<int32_t>(f, 8);
    const int n_kfs = h[0], n_kp = h[1], n_upd = h[2], n_rows = h[3], n_obs = h[4], what = h[5], nlevels = h[6], has_row = h[7];
    const auto kf_n = take<int32_t>(f, n_kfs), kf_bad = take<int32_t>(f, n_kfs), kf_first = take<int32_t>(f, n_kfs);
    const auto Ow = take<float>(f, 3 * (size_t)n_kfs);
    const auto desc = take<uint8_t>(f, 32 * (size_t)n_kp);
    const auto octave = take<int32_t>(f, n_kp);
    const auto row = take<int32_t>(f, has_row ? n_upd : 0);
    const auto obs_off = take<int32_t>(f, (size_t)n_upd + 1), obs_kf = take<int32_t>(f, n_obs), obs_idx = take<int32_t>(f, n_obs), ref = take<int32_t>(f, n_upd);
    const auto scale = take<float>(f, nlevels);
    const auto pos = take<float>(f, 3 * (size_t)n_rows);
    auto normal = take<float>(f, 3 * (size_t)n_rows), max_d = take<float>(f, n_rows), min_d = take<float>(f, n_rows);
    auto pt_desc = take<uint8_t>(f, 32 * (size_t)n_rows);
    fclose(f);

    std::vector<orbfe_keypoint> keys(n_kp);
    memset(keys.data(), 0, keys.size() * sizeof(orbfe_keypoint));
    for (int i = 0; i < n_kp; i++) keys[i].octave = octave[i];
    std::vector<orbfe_obs_keyframe> kfs(n_kfs);
    for (int k = 0; k < n_kfs; k++) {
        kfs[k].desc = desc.data() + 32 * (size_t)kf_first[k];
        kfs[k].keys_un = keys.data() + kf_first[k];
        for (int c = 0; c < 3; c++) kfs[k].Ow[c] = Ow[3 * (size_t)k + c];
        kfs[k].n = kf_n[k]; kfs[k].bad = kf_bad[k]; kfs[k].reserved = 0;
    }
    std::vector<int32_t> best(n_upd, -7);
    auto run = [&]() {
        return ORB_SLAM2::UpdateMapPoints(kfs.data(), n_kfs, n_upd, has_row ? row.data() : nullptr, n_rows, obs_off.data(), obs_kf.data(), obs_idx.data(), n_obs,
                                          ref.data(), what, scale.data(), nlevels, pos.data(), normal.data(), max_d.data(), min_d.data(), pt_desc.data(),
                                          best.data());
    };
    int32_t status = run();
    if (argc >= 5 && !strcmp(argv[3], "bench")) { // the update is idempotent on its own output: repeat it and report the fastest pass
        double fastest = 1e30;
        for (int k = 0; k < atoi(argv[4]); k++) {
            const auto t0 = std::chrono::steady_clock::now();
            status = run();
            const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
            if (us < fastest) fastest = us;
        }
        printf("host_update_us %.3f\n", fastest);
    }
    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    put(o, std::vector<int32_t>(1, status));
    put(o, best); put(o, normal); put(o, max_d); put(o, min_d); put(o, pt_desc);
    fclose(o);
    return 0;
}
