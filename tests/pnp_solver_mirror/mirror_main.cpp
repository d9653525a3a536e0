// mirror_main.cpp -- TEST-ONLY driver of orbslam2_amd/host/PnPsolver.h: reads the scenes that tests/test_pnp_solver_host.py writes, runs
// the host form on each and replays ORB_SLAM2::PnPsolver::iterate on its rows, and writes everything back.  Built twice with g++ through
// tests/host_forms.py, plain and with -fsanitize=address,undefined.
//   file:  int32 n_scenes;  per scene { int32 n_keys, n_kf, capacity, max_its, min_inliers, n_iterations, nlevels, table_max_its;  f32 epsilon,
//          th2;  f64 prob;  f32 cam[4], sigma2[nlevels];  keypoint keys[n_keys];  int32 f_match[n_keys];  f32 pos[n_kf][3];
//          int32 valid[n_kf];  uint32 draws[max_its][4] }
//          int32 n_replays;  per replay { int32 N, its_for_n, min_inliers, step, n_rows;  int32 counts[n_rows], ok[n_rows] }
//   out:   per scene { int32 status, n_corr, n_its, n_events, exhausted, table[capacity + 1], corr[capacity][2], sets[max_its][4],
//          events[max_its];  hypothesis hyp[max_its];  uint32 bits[max_its][words];  refined refined[max_its];
//          uint32 refined_bits[max_its][words];  3 x (steps 1, 5, 300) replay;  int32 continued_iterations, continued_rows }
//          per replay { replay }
//          replay = int32 calls;  calls x int32 { return, bNoMore, nInliers, inlier keypoints, iterations, best iteration }
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../orbslam2_amd/host/PnPsolver.h"

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

// the loop of src/Tracking.cc:1497-1600 for one solver: iterate(step) until bNoMore
static void replay(FILE *o, const ORB_SLAM2::PnPRows &rows, int n_keys, int its, int min_inliers, float epsilon, int step)
{
    ORB_SLAM2::PnPsolver solver(&rows, n_keys, its, min_inliers, epsilon);
    std::vector<int32_t> log;
    int calls = 0;
    bool bNoMore = false;
    while (!bNoMore && calls < 4096) {
        std::vector<bool> inl;
        int nInliers = 0;
        const int r = solver.iterate(step, bNoMore, inl, nInliers);
        int slots = 0;
        for (bool b : inl) slots += b;
        if ((r == ORB_SLAM2::PnPsolver::kNone) != (solver.GetPose() == nullptr)) { fprintf(stderr, "GetPose\n"); exit(3); }
        log.insert(log.end(), {r, (int32_t)bNoMore, nInliers, slots, solver.Iterations(), solver.BestIteration()});
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
        const int n_keys = h[0], n_kf = h[1], capacity = h[2], max_its = h[3], min_inliers = h[4], n_iterations = h[5], nlevels = h[6], table_max_its = h[7];
        const auto fl = take<float>(f, 2);
        const double prob = take<double>(f, 1)[0];
        const auto cam = take<float>(f, 4), sigma2 = take<float>(f, nlevels);
        const auto keys = take<orbfe_keypoint>(f, n_keys);
        const auto f_match = take<int32_t>(f, n_keys);
        const auto pos = take<float>(f, 3 * (size_t)n_kf);
        const auto valid = take<int32_t>(f, n_kf);
        const auto draws = take<uint32_t>(f, 4 * (size_t)max_its);
        const std::vector<int32_t> table = PnPRansacIterationTable(capacity, prob, min_inliers, table_max_its, fl[0]);
        PnPProblem problem;
        const PnPRows rows = PnPRansacHost(keys.data(), n_keys, f_match.data(), pos.data(), valid.data(), n_kf, draws.data(), capacity, min_inliers, max_its,
                                           n_iterations, fl[0], fl[1], table.data(), sigma2.data(), nlevels, cam.data(), &problem);
        put(o, std::vector<int32_t>{rows.status, rows.n_corr, rows.n_its, rows.n_events, rows.exhausted});
        put(o, table); put(o, rows.corr); put(o, rows.sets); put(o, rows.events); put(o, rows.hyp); put(o, rows.bits); put(o, rows.refined);
        put(o, rows.refined_bits);
        // replayed on a copy made the way rows fetched from the device are handed over
        const PnPRows again = PnPRowsOfCandidate(0, capacity, max_its, &rows.status, &rows.n_corr, &rows.n_its, &rows.n_events, &rows.exhausted, rows.events.data(),
                                                 rows.hyp.data(), rows.refined.data(), rows.corr.data(), rows.bits.data(), rows.refined_bits.data());
        for (int step : {1, 5, 300}) replay(o, again, n_keys, table[rows.n_corr], min_inliers, fl[0], step);
        // a solver with the problem continues beyond its rows with the host form: three further calls of iterate(5)
        PnPsolver solver(&again, n_keys, table[rows.n_corr], min_inliers, fl[0], &problem);
        int before = 0, after = 0;
        if (rows.n_its > 0) {
            bool bNoMore = false;
            std::vector<bool> inl;
            int nInliers = 0;
            while (!bNoMore && solver.Iterations() < rows.n_its) solver.iterate(5, bNoMore, inl, nInliers);
            before = solver.Iterations();
            for (int c = 0; c < 3; c++) solver.iterate(5, bNoMore, inl, nInliers);
            after = solver.Iterations();
        }
        put(o, std::vector<int32_t>{before, after});
    }
    const int n_replays = take<int32_t>(f, 1)[0];
    for (int q = 0; q < n_replays; q++) { // hand-written rows: counts and whether a record holder's refinement succeeds
        const auto h = take<int32_t>(f, 5);
        const auto counts = take<int32_t>(f, h[4]);
        const auto ok = take<int32_t>(f, h[4]);
        PnPRows rows;
        PnPRowsInit(rows, std::max(h[0], 1), std::max(h[4], 1));
        rows.n_corr = h[0]; rows.n_its = h[4];
        int best = 0, best_k = -1;
        for (int k = 0; k < h[4]; k++) {
            rows.hyp[k].n_inliers = counts[k];
            if (counts[k] >= h[2]) {
                if (counts[k] > best) { best = counts[k]; best_k = k; rows.refined[k].ok = ok[k]; rows.refined[k].n_inliers = counts[k]; }
                if (rows.refined[best_k].ok) rows.events[rows.n_events++] = k;
            }
            rows.hyp[k].best_k = best_k;
        }
        rows.exhausted = best_k;
        replay(o, rows, 1, h[1], h[2], 0.f, h[3]);
    }
    fclose(f);
    fclose(o);
    return 0;
}
