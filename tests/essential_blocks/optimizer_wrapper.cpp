// TEST-ONLY: ORB_SLAM2::Optimizer::EssentialGraphEdges and ::OptimizeEssentialGraph of orbslam2_amd/host/Optimizer.h behind C functions, so
// that tests/test_essential_graph_edges.py and tests/test_essential_graph_device.py can call the header's wrappers (std::vector in,
// exception on error) from Python.  Nested lists arrive as CSR: off[k] .. off[k + 1] - 1 of the value array.
#include <cstdint>
#include <exception>
#include <vector>

#include "../../orbslam2_amd/host/Optimizer.h"

namespace {
std::vector<std::vector<int32_t>> lists(int n, const int32_t *off, const int32_t *val)
{
    std::vector<std::vector<int32_t>> out(n);
    for (int k = 0; k < n; k++) out[k].assign(val + off[k], val + off[k + 1]);
    return out;
}
} // namespace

// returns the number of edges (written up to `capacity`), or -100 when the wrapper threw
extern "C" int eg_wrapper_edges(int n_kfs, const uint64_t *id, const int32_t *parent, const int32_t *loop_off, const int32_t *loop_val, const int32_t *cov_off,
                                const int32_t *cov_val, const int32_t *child_off, const int32_t *child_val, int n_conn, const int32_t *conn_kf,
                                const int32_t *conn_off, const int32_t *conn_val, const int32_t *conn_weight, int min_feat, int cur_kf, int loop_kf,
                                int32_t *edge_i, int32_t *edge_j, uint8_t *edge_kind, int capacity)
{
    try {
        std::vector<ORB_SLAM2::Optimizer::LoopConnection> conn(n_conn);
        for (int c = 0; c < n_conn; c++) {
            conn[c].kf = conn_kf[c];
            conn[c].vConnected.assign(conn_val + conn_off[c], conn_val + conn_off[c + 1]);
            conn[c].vWeight.assign(conn_weight + conn_off[c], conn_weight + conn_off[c + 1]);
        }
        const std::vector<unsigned long> ids(id, id + n_kfs);
        const std::vector<int32_t> par(parent, parent + n_kfs);
        const auto edges = ORB_SLAM2::Optimizer::EssentialGraphEdges(ids, par, lists(n_kfs, loop_off, loop_val), lists(n_kfs, cov_off, cov_val),
                                                                    lists(n_kfs, child_off, child_val), conn, min_feat, cur_kf, loop_kf);
        for (size_t e = 0; e < edges.size() && (int)e < capacity; e++) { edge_i[e] = edges[e].i; edge_j[e] = edges[e].j; edge_kind[e] = edges[e].kind; }
        return (int)edges.size();
    } catch (const std::exception &) {
        return -100;
    }
}

// 0 on success; -100 when the wrapper threw
extern "C" int eg_wrapper_optimize(orbfe_context *ctx, int n_kfs, int loop_kf, float *Tcw, float *Ow, const int32_t *edge_i, const int32_t *edge_j,
                                   const uint8_t *edge_kind, int n_edges, const double *corrected, const uint8_t *has_corrected, const double *noncorrected,
                                   const uint8_t *has_noncorrected, float *pos, const int32_t *pt_ref, const uint8_t *pt_valid, int n_pts, int fix_scale,
                                   int iterations, uint8_t *edge_code, uint8_t *pt_code, double *sim3, orbfe_essential_graph_info *info, int32_t *status)
{
    try {
        std::vector<float> vT(Tcw, Tcw + 16 * (size_t)n_kfs), vOw, vP(pos, pos + 3 * (size_t)n_pts);
        std::vector<ORB_SLAM2::Optimizer::EssentialEdge> edges(n_edges);
        for (int e = 0; e < n_edges; e++) edges[e] = {edge_i[e], edge_j[e], edge_kind[e]};
        const std::vector<double> co = corrected ? std::vector<double>(corrected, corrected + 8 * (size_t)n_kfs) : std::vector<double>();
        const std::vector<uint8_t> hc = corrected ? std::vector<uint8_t>(has_corrected, has_corrected + n_kfs) : std::vector<uint8_t>();
        const std::vector<double> no = noncorrected ? std::vector<double>(noncorrected, noncorrected + 8 * (size_t)n_kfs) : std::vector<double>();
        const std::vector<uint8_t> hn = noncorrected ? std::vector<uint8_t>(has_noncorrected, has_noncorrected + n_kfs) : std::vector<uint8_t>();
        const std::vector<int32_t> ref(pt_ref, pt_ref + n_pts);
        const std::vector<uint8_t> valid(pt_valid, pt_valid + n_pts);
        const auto r = ORB_SLAM2::Optimizer::OptimizeEssentialGraph(ctx, vT, vOw, loop_kf, edges, co, hc, no, hn, vP, ref, valid, fix_scale != 0, iterations);
        for (size_t k = 0; k < vT.size(); k++) Tcw[k] = vT[k];
        for (size_t k = 0; k < vOw.size(); k++) Ow[k] = vOw[k];
        for (size_t k = 0; k < vP.size(); k++) pos[k] = vP[k];
        for (int e = 0; e < n_edges; e++) edge_code[e] = r.vEdgeCode[e];
        for (int q = 0; q < n_pts; q++) pt_code[q] = r.vPointCode[q];
        for (size_t k = 0; k < r.vSim3.size(); k++) sim3[k] = r.vSim3[k];
        *info = r.info;
        *status = r.status;
        return 0;
    } catch (const std::exception &) {
        return -100;
    }
}
