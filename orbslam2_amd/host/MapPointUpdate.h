// MapPointUpdate.h -- MapPoint::ComputeDistinctiveDescriptors (reference src/MapPoint.cc:242-307) and MapPoint::UpdateNormalAndDepth
// (:330-371) restated on the flat arrays of orbfe_enqueue_update_map_points (include/orbfe.h), in plain C++ on the host: the same
// arguments, but every pointer (those inside the orbfe_obs_keyframe records too) is a HOST pointer and the scale factors are passed in.
// Header-only, no library and no device needed.  It is
//   - the form for callers without a device store (the synchronous counterpart of the enqueue call),
//   - written literally -- the N x N distance matrix, the sorted vDists, the strict < -- so that it is a second formulation next to
//     the kernel's sort-free bisection, and
//   - the host leg of tools/bench_matchers.py --map-points.
// Compile with -ffp-contract=off: every float operation below is rounded once (contract Q4), as in the kernel.
#pragma once

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/orbfe.h"
#include "CvMat.h"

namespace ORB_SLAM2
{

// ORBmatcher::DescriptorDistance: the Hamming distance of two 32-byte descriptors, taken as eight 32-bit words
inline int MapPointDescriptorDistance(const uint8_t *a, const uint8_t *b)
{
    int dist = 0;
    for (int i = 0; i < 8; i++) {
        uint32_t wa, wb;
        std::memcpy(&wa, a + 4 * i, 4);
        std::memcpy(&wb, b + 4 * i, 4);
        dist += __builtin_popcount(wa ^ wb);
    }
    return dist;
}

// Returns 0, or ORBFE_ERR_INVALID when an update was faulty (what the device reports in d_status: that update is skipped whole, its
// best entry is -1, every other update is unaffected) or an argument is refused (then nothing is written).
inline int UpdateMapPoints(const orbfe_obs_keyframe *kfs, int n_kfs, int n_upd, const int32_t *row, int n_rows, const int32_t *obs_off,
                           const int32_t *obs_kf, const int32_t *obs_idx, int n_obs, const int32_t *ref, int what, const float *scale, int nlevels,
                           const float *pos, float *normal, float *max_distance, float *min_distance, uint8_t *pt_desc, int32_t *best)
{
    const bool desc = (what & ORBFE_MP_DESCRIPTOR) != 0, nd = (what & ORBFE_MP_NORMAL_DEPTH) != 0;
    if (n_kfs < 0 || n_upd < 0 || n_rows < 0 || n_obs < 0 || what < 1 || what > 3 || nlevels < 1 || (!row && n_rows < n_upd)) return ORBFE_ERR_INVALID;
    if (n_upd > 0 && (!obs_off || !pos || !scale || (desc && !pt_desc) || (nd && (!normal || !max_distance || !min_distance || !ref)) ||
                      (n_obs > 0 && (!kfs || !obs_kf || !obs_idx))))
        return ORBFE_ERR_INVALID;
    int status = 0;
    std::vector<const uint8_t *> vDescriptors;
    std::vector<int> vListPos, Distances, vDists;
    for (int q = 0; q < n_upd; q++) {
        if (best) best[q] = -1;
        const int r = row ? row[q] : q;
        const int o0 = obs_off[q], o1 = obs_off[q + 1];
        bool fault = r < 0 || r >= n_rows || o0 < 0 || o1 < o0 || o1 > n_obs;
        for (int o = o0; !fault && o < o1; o++)
            fault = obs_kf[o] < 0 || obs_kf[o] >= n_kfs || obs_idx[o] < 0 || obs_idx[o] >= kfs[obs_kf[o]].n || !kfs[obs_kf[o]].desc;
        int level = 0;
        if (!fault && nd && o1 > o0) {
            fault = ref[q] < 0 || ref[q] >= o1 - o0 || !kfs[obs_kf[o0 + ref[q]]].keys_un;
            if (!fault) {
                level = kfs[obs_kf[o0 + ref[q]]].keys_un[obs_idx[o0 + ref[q]]].octave;
                fault = level < 0 || level >= nlevels;
            }
        }
        if (fault) { status = ORBFE_ERR_INVALID; continue; }
        if (o1 == o0) continue; // observations.empty()

        if (desc) {
            // Retrieve all observed descriptors
            vDescriptors.clear(); vListPos.clear();
            for (int o = o0; o < o1; o++) {
                const orbfe_obs_keyframe &kf = kfs[obs_kf[o]];
                if (!kf.bad) { vDescriptors.push_back(kf.desc + (size_t)obs_idx[o] * 32); vListPos.push_back(o - o0); }
            }
            if (!vDescriptors.empty()) {
                // Compute distances between them
                const size_t N = vDescriptors.size();
                Distances.assign(N * N, 0);
                for (size_t i = 0; i < N; i++) {
                    Distances[i * N + i] = 0;
                    for (size_t j = i + 1; j < N; j++) {
                        const int distij = MapPointDescriptorDistance(vDescriptors[i], vDescriptors[j]);
                        Distances[i * N + j] = distij;
                        Distances[j * N + i] = distij;
                    }
                }
                // Take the descriptor with least median distance to the rest
                int BestMedian = INT_MAX;
                int BestIdx = 0;
                for (size_t i = 0; i < N; i++) {
                    vDists.assign(Distances.begin() + i * N, Distances.begin() + (i + 1) * N);
                    std::sort(vDists.begin(), vDists.end());
                    const int median = vDists[(size_t)(0.5 * (N - 1))];
                    if (median < BestMedian) {
                        BestMedian = median;
                        BestIdx = (int)i;
                    }
                }
                std::memcpy(pt_desc + (size_t)r * 32, vDescriptors[BestIdx], 32);
                if (best) best[q] = vListPos[BestIdx];
            }
        }

        if (nd) {
            const float *Pos = pos + 3 * (size_t)r;
            float acc[3] = {0.f, 0.f, 0.f};
            int n = 0;
            for (int o = o0; o < o1; o++) {
                const float *Owi = kfs[obs_kf[o]].Ow;
                const float normali[3] = {Pos[0] - Owi[0], Pos[1] - Owi[1], Pos[2] - Owi[2]};
                const float alpha = (float)(1.0 / Norm3(normali)); // Mat / double is a scale by 1./s; scaleAdd takes the factor as float
                for (int c = 0; c < 3; c++) {
                    const float term = normali[c] * alpha;
                    acc[c] = term + acc[c];
                }
                n++;
            }
            const float *Owr = kfs[obs_kf[o0 + ref[q]]].Ow;
            const float PC[3] = {Pos[0] - Owr[0], Pos[1] - Owr[1], Pos[2] - Owr[2]};
            const float dist = (float)Norm3(PC);
            const float inv_n = (float)(1.0 / (double)n); // Mat / int: convertTo with a float scale
            max_distance[r] = dist * scale[level];
            min_distance[r] = max_distance[r] / scale[nlevels - 1];
            for (int c = 0; c < 3; c++) normal[3 * (size_t)r + c] = acc[c] * inv_n;
        }
    }
    return status;
}

} // namespace ORB_SLAM2
