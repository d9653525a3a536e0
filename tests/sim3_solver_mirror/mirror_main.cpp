// mirror_main.cpp -- TEST-ONLY driver of orbslam2_amd/host/Sim3Solver.h: reads the scenes that tests/test_sim3_solver_host.py writes, runs
// the host form on each and replays ORB_SLAM2::Sim3Solver::iterate on its rows, and writes everything back.  Built twice with g++ through
// tests/host_forms.py, plain and with -fsanitize=address,undefined.
//   file:  int32 n_scenes;  per scene { int32 n1, n2, n_pairs, max_pairs, max_its, min_inliers, fix_scale, nlevels;  f64 prob;  f32 cam[4],
//          sigma2[nlevels], T1w[12], T2w[12];  keypoint keys1[n1];  f32 pos1[n1][3];  int32 valid1[n1];  the same of KF2;
//          int32 pairs[n_pairs][2];  uint32 draws[max_its][3] }
//          int32 n_replays;  per replay { int32 N, n_its, min_inliers, step, n_counts;  int32 counts[n_counts] }
//   out:   per scene { int32 status, n_corr, n_its, n_events, table[max_pairs + 1], corr[max_pairs][2], sets[max_its][3], events[max_its];
//          hypothesis hyp[max_its];  uint32 bits[max_its][words];  3 x (steps 1, 5, 300) { int32 calls;  calls x int32 { k, bNoMore, nInliers,
//          inlier slots, iterations } } }
//          per replay { int32 calls;  calls x int32 { k, bNoMore, nInliers, 0, iterations } }
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../orbslam2_amd/host/Sim3Solver.h"

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

// the loop of src/LoopClosing.cc:322-378 for one solver: iterate(step) until bNoMore
static void replay(FILE *o, const ORB_SLAM2::Sim3Rows &rows, int n1, int min_inliers, int step)
{
    ORB_SLAM2::Sim3Solver solver(&rows, n1, min_inliers);
    std::vector<int32_t> log;
    int calls = 0;
    bool bNoMore = false;
    while (!bNoMore && calls < 4096) {
        std::vector<bool> inl;
        int nInliers = 0;
        const int k = solver.iterate(step, bNoMore, inl, nInliers);
        int slots = 0;
        for (bool b : inl) slots += b;
        if (k >= 0 && solver.GetEstimatedScale() != rows.hyp[k].s12 && rows.hyp[k].s12 == rows.hyp[k].s12) { fprintf(stderr, "GetEstimatedScale\n"); exit(3); }
        log.insert(log.end(), {k, (int32_t)bNoMore, nInliers, slots, solver.Iterations()});
        calls++;
    }
    put(o, std::vector<int32_t>{calls});
    put(o, log);
}

int main(int argc, char **argv)
{
    using namespace ORB_SLAM2;
    if (argc < 3) { fprintf(stderr, "usage: %s problem.bin out.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    const int n_scenes = take<int32_t>(f, 1)[0];
    for (int q = 0; q < n_scenes; q++) {
        const auto h = take<int32_t>(f, 8);
        const int n1 = h[0], n2 = h[1], n_pairs = h[2], max_pairs = h[3], max_its = h[4], min_inliers = h[5], fix_scale = h[6], nlevels = h[7];
        const double prob = take<double>(f, 1)[0];
        const auto cam = take<float>(f, 4), sigma2 = take<float>(f, nlevels), T1w = take<float>(f, 12), T2w = take<float>(f, 12);
        const auto keys1 = take<orbfe_keypoint>(f, n1);
        const auto pos1 = take<float>(f, 3 * (size_t)n1);
        const auto valid1 = take<int32_t>(f, n1);
        const auto keys2 = take<orbfe_keypoint>(f, n2);
        const auto pos2 = take<float>(f, 3 * (size_t)n2);
        const auto valid2 = take<int32_t>(f, n2);
        const auto pairs = take<int32_t>(f, 2 * (size_t)n_pairs);
        const auto draws = take<uint32_t>(f, 3 * (size_t)max_its);
        const std::vector<int32_t> table = Sim3RansacIterationTable(max_pairs, prob, min_inliers, max_its);
        const Sim3Rows rows = Sim3RansacHost(keys1.data(), n1, T1w.data(), pos1.data(), valid1.data(), keys2.data(), n2, T2w.data(), pos2.data(), valid2.data(),
                                             pairs.data(), n_pairs, draws.data(), max_pairs, fix_scale, min_inliers, max_its, table.data(), sigma2.data(), nlevels,
                                             cam.data());
        put(o, std::vector<int32_t>{rows.status, rows.n_corr, rows.n_its, rows.n_events});
        put(o, table); put(o, rows.corr); put(o, rows.sets); put(o, rows.events); put(o, rows.hyp); put(o, rows.bits);
        // replayed on a copy made the way rows fetched from the device are handed over
        const Sim3Rows again = Sim3RowsOfCandidate(0, max_pairs, max_its, &rows.status, &rows.n_corr, &rows.n_its, &rows.n_events, rows.events.data(),
                                                   rows.hyp.data(), rows.corr.data(), rows.bits.data());
        for (int step : {1, 5, 300}) replay(o, again, n1, min_inliers, step);
    }
    const int n_replays = take<int32_t>(f, 1)[0];
    for (int q = 0; q < n_replays; q++) { // hand-written count sequences: the rows hold nothing but counts and their events
        const auto h = take<int32_t>(f, 5);
        const auto counts = take<int32_t>(f, h[4]);
        Sim3Rows rows;
        rows.n_corr = h[0]; rows.n_its = h[1]; rows.max_its = h[4]; rows.max_pairs = std::max(h[0], 1); rows.words = (rows.max_pairs + 31) / 32;
        rows.corr.assign(2 * (size_t)rows.max_pairs, 0);
        rows.hyp.assign(h[4], orbfe_sim3_hypothesis());
        rows.bits.assign((size_t)h[4] * rows.words, 0u);
        rows.events.assign(h[4], -1);
        int best = 0;
        for (int k = 0; k < h[1]; k++) {
            rows.hyp[k].n_inliers = counts[k];
            if (counts[k] >= best) { best = counts[k]; if (counts[k] > h[2]) rows.events[rows.n_events++] = k; }
        }
        replay(o, rows, 1, h[2], h[3]);
    }
    fclose(f);
    fclose(o);
    return 0;
}
