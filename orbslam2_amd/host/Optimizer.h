// Optimizer.h -- host-side mirror of ORB_SLAM2::Optimizer::PoseOptimization (reference include/Optimizer.h:48,
// src/Optimizer.cc:283-495) and Optimizer::OptimizeSim3 over the C ABI (include/orbfe.h).  The reference takes a Frame*; this mirror takes the
// fields of the Frame it reads and writes, flattened:
//   reads   mTcw, N, mvKeysUn, mvuRight, mvpMapPoints[i] != NULL and GetWorldPos() of those, mvInvLevelSigma2 / fx, fy,
//           cx, cy, mbf (taken from the context the extractor of this camera was built with)
//   writes  mvbOutlier (entries that hold a map point), the pose handed to SetPose, and returns the inlier count
// A drop-in Optimizer::PoseOptimization(Frame *pFrame) gathers those fields, calls this, and finishes with
// pFrame->SetPose(cv::Mat(4, 4, CV_32F, Tcw).clone()) when at least 3 correspondences existed.
//
// Optimizer::OptimizeSim3 (include/Optimizer.h, src/Optimizer.cc:1090-1285) likewise, on the fields of the two keyframes it reads:
//   reads   GetRotation() / GetTranslation() of both (T1w, T2w: 3x4 row major), mvKeysUn, per keypoint slot GetWorldPos() of its map point
//           and pMP && !pMP->isBad(); vpMatches1 as keypoint slots of KF2 (-1: none); the Sim3 as LoopClosing::ComputeSim3 builds it
//           (s, R, t of the Sim3Solver: floats); th2, bFixScale
//   writes  vnMatches12 (outliers become -1), S12 = qx qy qz qw tx ty tz s of the optimised g2o::Sim3 (the input one when the
//           optimisation gives up), and returns nIn
//
// Optimizer::LocalBundleAdjustment (include/Optimizer.h, src/Optimizer.cc:497-822) likewise, after its graph walk (:499-548), which stays
// the caller's and arrives flattened:
//   reads   per keyframe of lLocalKeyFrames / lFixedCameras (and of any other keyframe an observation names) mvKeysUn, mvuRight, GetPose()
//           and its role: ORBFE_BA_LOCAL, ORBFE_BA_LOCAL_HELD (mnId == 0), ORBFE_BA_FIXED, ORBFE_BA_SKIP (isBad()); per point of
//           lLocalMapPoints GetWorldPos() and GetObservations() as (keyframe index, keypoint index) in mObservations' order
//   writes  the poses handed to SetPose (roles 1 and 2) with their camera centres, the positions handed to SetWorldPos, vToErase as
//           (keyframe index, point index) pairs in the reference's order; returns the call's orbfe_lba_info
// pbStopFlag is not restated: the call cannot be interrupted (include/orbfe.h).  UpdateNormalAndDepth stays a call of its own
// (MapPointUpdate.h) because erasing an observation can change mpRefKF or kill the point.
//
// Optimizer::OptimizeEssentialGraph (include/Optimizer.h, src/Optimizer.cc:825-1088) likewise, in two steps.  EssentialGraphEdges restates
// the edge walk of :891-1027 on flattened fields; keyframes are indices into vpKFs = pMap->GetAllKeyFrames() without the bad ones, in the
// caller's iteration order (the reference iterates std::set<KeyFrame*> and std::map<KeyFrame*, ...>: pointer order, which the caller keeps):
//   reads   mnId, GetParent(), GetLoopEdges(), GetCovisiblesByWeight(minFeat) (-1 for an entry that isBad()), GetChilds(), LoopConnections
//           with pKF->GetWeight() of every connection, minFeat, pCurKF, pLoopKF
//   writes  (i, j, kind) per edge in the reference's insertion order: vertex 0 = i, vertex 1 = j, kind 0 for a LoopConnections edge
// OptimizeEssentialGraph then takes those edges with GetPose() of every keyframe, CorrectedSim3 / NonCorrectedSim3 as eight doubles and a
// flag per keyframe, GetWorldPos() of every map point with the keyframe whose Sim3s move it and !isBad(); it writes the poses handed to
// SetPose with their camera centres and the positions handed to SetWorldPos.  UpdateNormalAndDepth stays MapPointUpdate.h's call.
#pragma once

#include <algorithm>
#include <cstdint>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/orbfe.h"

namespace ORB_SLAM2
{

class Optimizer
{
public:
    // returns nInitialCorrespondences - nBad; Tcw (16 floats, row major) and vbOutlier are updated in place
    static int PoseOptimization(orbfe_context *ctx, float *Tcw, const std::vector<orbfe_keypoint> &vKeysUn,
                                const std::vector<float> &vuRight, const std::vector<uint8_t> &vbHasMapPoint,
                                const std::vector<float> &vWorldPos /* 3 per keypoint */, std::vector<uint8_t> &vbOutlier)
    {
        const size_t N = vKeysUn.size();
        if (vuRight.size() != N || vbHasMapPoint.size() != N || vWorldPos.size() != 3 * N)
            throw std::invalid_argument("Optimizer::PoseOptimization: per-keypoint arrays differ in length");
        vbOutlier.resize(N, 0);
        int nInliers = 0;
        const int rc = orbfe_pose_optimization(ctx, Tcw, (int)N, vKeysUn.data(), vuRight.data(), vbHasMapPoint.data(), vWorldPos.data(),
                                               vbOutlier.data(), &nInliers);
        if (rc != ORBFE_OK) throw std::runtime_error(std::string("orbfe: ") + orbfe_last_error(ctx));
        return nInliers;
    }

    // returns nIn; vnMatches12 (one entry per keypoint of KF1) is updated in place, S12 receives eight doubles.  vnPrior12 may be empty:
    // otherwise its entries >= 0 take precedence over vnMatches12's (the RANSAC inliers, src/LoopClosing.cc:343-353).
    static int OptimizeSim3(orbfe_context *ctx, const std::vector<orbfe_keypoint> &vKeysUn1, const float *T1w, const std::vector<float> &vWorldPos1 /* 3 per keypoint */,
                            const std::vector<int32_t> &vbValid1, const std::vector<orbfe_keypoint> &vKeysUn2, const float *T2w,
                            const std::vector<float> &vWorldPos2, const std::vector<int32_t> &vbValid2, float s12, const float *R12, const float *t12,
                            std::vector<int32_t> &vnMatches12, double *S12, float th2, bool bFixScale, const std::vector<int32_t> &vnPrior12 = std::vector<int32_t>(),
                            const orbfe_sim3_opt_params *params = nullptr)
    {
        const size_t N1 = vKeysUn1.size(), N2 = vKeysUn2.size();
        if (vWorldPos1.size() != 3 * N1 || vbValid1.size() != N1 || vnMatches12.size() != N1 || vWorldPos2.size() != 3 * N2 || vbValid2.size() != N2 ||
            (!vnPrior12.empty() && vnPrior12.size() != N1))
            throw std::invalid_argument("Optimizer::OptimizeSim3: per-keypoint arrays differ in length");
        int nIn = 0;
        const int rc = orbfe_optimize_sim3(ctx, vKeysUn1.data(), (int)N1, T1w, vWorldPos1.data(), vbValid1.data(), vKeysUn2.data(), (int)N2, T2w,
                                           vWorldPos2.data(), vbValid2.data(), s12, R12, t12, th2, bFixScale ? 1 : 0, params,
                                           vnPrior12.empty() ? nullptr : vnPrior12.data(), vnMatches12.data(), S12, &nIn);
        if (rc != ORBFE_OK) throw std::runtime_error(std::string("orbfe: ") + orbfe_last_error(ctx));
        return nIn;
    }

    struct BAKeyFrame { // what the call reads of one keyframe
        const std::vector<orbfe_keypoint> *vKeysUn;
        const std::vector<float> *vuRight;
        uint8_t role; // ORBFE_BA_*
    };
    struct BAResult {
        std::vector<std::pair<int32_t, int32_t>> vToErase; // (keyframe index, point index)
        std::vector<uint8_t> vEdgeCode;                    // per observation: 1 level 1 in round 2, 2 erased, 4 skipped
        std::vector<double> vEdgeChi2;
        orbfe_lba_info info;
    };

    // vTcw (16 floats per keyframe, row major) and vWorldPos (3 per point) are updated in place; vOw (3 per keyframe, resized when it
    // is shorter) receives the camera centre of every rewritten keyframe (roles 1 and 2); the rows of the other keyframes keep what the
    // caller put there (zeros where the resize added them).  vObsOff (one more entry than points), vObsKF, vObsIdx: the points' observations.
    static BAResult LocalBundleAdjustment(orbfe_context *ctx, const std::vector<BAKeyFrame> &vKFs, std::vector<float> &vTcw, std::vector<float> &vOw,
                                          std::vector<float> &vWorldPos, const std::vector<int32_t> &vObsOff, const std::vector<int32_t> &vObsKF,
                                          const std::vector<int32_t> &vObsIdx)
    {
        const size_t K = vKFs.size(), E = vObsKF.size();
        if (vObsOff.empty() || vTcw.size() != 16 * K || vWorldPos.size() != 3 * (vObsOff.size() - 1) || vObsIdx.size() != E)
            throw std::invalid_argument("Optimizer::LocalBundleAdjustment: arrays differ in length");
        const size_t N = vObsOff.size() - 1;
        std::vector<const orbfe_keypoint *> keys(K);
        std::vector<const float *> ur(K);
        std::vector<int32_t> n(K);
        std::vector<uint8_t> role(K);
        for (size_t k = 0; k < K; k++) {
            if (vKFs[k].vKeysUn->size() != vKFs[k].vuRight->size()) throw std::invalid_argument("Optimizer::LocalBundleAdjustment: mvKeysUn and mvuRight differ in length");
            keys[k] = vKFs[k].vKeysUn->data(); ur[k] = vKFs[k].vuRight->data(); n[k] = (int32_t)vKFs[k].vKeysUn->size(); role[k] = vKFs[k].role;
        }
        vOw.resize(3 * K);
        BAResult r;
        r.vEdgeCode.assign(E, 0);
        r.vEdgeChi2.assign(E, 0.0);
        std::vector<int32_t> erase(2 * E + 2);
        int32_t n_erase = 0;
        const int rc = orbfe_local_bundle_adjustment(ctx, keys.data(), ur.data(), n.data(), role.data(), (int)K, vTcw.data(), (int)N, nullptr, (int)N,
                                                     vObsOff.data(), vObsKF.data(), vObsIdx.data(), (int)E, vWorldPos.data(), vOw.data(),
                                                     r.vEdgeCode.data(), r.vEdgeChi2.data(), erase.data(), &n_erase, &r.info);
        if (rc != ORBFE_OK) throw std::runtime_error(std::string("orbfe: ") + orbfe_last_error(ctx));
        for (int32_t i = 0; i < n_erase; i++) r.vToErase.emplace_back(erase[2 * i], erase[2 * i + 1]);
        return r;
    }

    struct EssentialEdge { int32_t i, j; uint8_t kind; };
    struct LoopConnection { // one entry of LoopConnections: mit->first, then mit->second in its iteration order with pKF->GetWeight(*sit)
        int32_t kf;
        std::vector<int32_t> vConnected;
        std::vector<int> vWeight;
    };

    // The edge walk of :891-1027.  vCovisibles[i] = GetCovisiblesByWeight(minFeat) of keyframe i, -1 where the entry isBad().
    static std::vector<EssentialEdge> EssentialGraphEdges(const std::vector<unsigned long> &vnId, const std::vector<int32_t> &vnParent,
                                                          const std::vector<std::vector<int32_t>> &vLoopEdges, const std::vector<std::vector<int32_t>> &vCovisibles,
                                                          const std::vector<std::vector<int32_t>> &vChildren, const std::vector<LoopConnection> &vLoopConnections,
                                                          int minFeat, int32_t nCurKF, int32_t nLoopKF)
    {
        const size_t K = vnId.size();
        if (vnParent.size() != K || vLoopEdges.size() != K || vCovisibles.size() != K || vChildren.size() != K)
            throw std::invalid_argument("Optimizer::EssentialGraphEdges: per-keyframe arrays differ in length");
        auto inside = [K](int32_t v) { return v >= 0 && (size_t)v < K; };
        if (!inside(nCurKF) || !inside(nLoopKF)) throw std::invalid_argument("Optimizer::EssentialGraphEdges: pCurKF / pLoopKF outside the map");
        std::vector<EssentialEdge> out;
        std::set<std::pair<unsigned long, unsigned long>> sInsertedEdges;
        // Set Loop edges (:896-924)
        for (const LoopConnection &c : vLoopConnections) {
            if (!inside(c.kf) || c.vConnected.size() != c.vWeight.size()) throw std::invalid_argument("Optimizer::EssentialGraphEdges: a faulty loop connection");
            const unsigned long nIDi = vnId[c.kf];
            for (size_t k = 0; k < c.vConnected.size(); k++) {
                const int32_t j = c.vConnected[k];
                if (!inside(j)) throw std::invalid_argument("Optimizer::EssentialGraphEdges: a loop connection outside the map");
                const unsigned long nIDj = vnId[j];
                if ((nIDi != vnId[nCurKF] || nIDj != vnId[nLoopKF]) && c.vWeight[k] < minFeat) continue;
                out.push_back({c.kf, j, 0});
                sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
            }
        }
        // Set normal edges (:927-1027)
        for (size_t i = 0; i < K; i++) {
            const int32_t parent = vnParent[i];
            if (parent >= 0) { // Spanning tree edge
                if (!inside(parent)) throw std::invalid_argument("Optimizer::EssentialGraphEdges: a parent outside the map");
                out.push_back({(int32_t)i, parent, 1});
            }
            for (int32_t l : vLoopEdges[i]) { // Loop edges
                if (!inside(l)) throw std::invalid_argument("Optimizer::EssentialGraphEdges: a loop edge outside the map");
                if (vnId[l] < vnId[i]) out.push_back({(int32_t)i, l, 1});
            }
            for (int32_t n : vCovisibles[i]) { // Covisibility graph edges
                if (n < 0) continue; // isBad()
                if (!inside(n)) throw std::invalid_argument("Optimizer::EssentialGraphEdges: a covisible keyframe outside the map");
                const bool child = std::find(vChildren[i].begin(), vChildren[i].end(), n) != vChildren[i].end();
                const bool loop = std::find(vLoopEdges[i].begin(), vLoopEdges[i].end(), n) != vLoopEdges[i].end();
                if (n == parent || child || loop) continue;
                if (vnId[n] < vnId[i]) {
                    if (sInsertedEdges.count(std::make_pair(std::min(vnId[i], vnId[n]), std::max(vnId[i], vnId[n])))) continue;
                    out.push_back({(int32_t)i, n, 1});
                }
            }
        }
        return out;
    }

    struct EssentialGraphResult {
        std::vector<uint8_t> vEdgeCode, vPointCode; // ORBFE_EG_EDGE_*; 1 for a point whose keyframe index is outside the map
        std::vector<double> vSim3;                  // the optimised Sim3 of every keyframe, eight doubles each
        orbfe_essential_graph_info info;
        int32_t status;                             // 0, or ORBFE_ERR_INVALID when a code was set
    };

    // vTcw (16 floats per keyframe) and vWorldPos (3 per point) are updated in place, vOw (3 per keyframe) receives the camera centres.
    // vCorrected / vNonCorrected: eight doubles per keyframe (qx qy qz qw tx ty tz s) where the flag is set; both pairs may be empty.
    static EssentialGraphResult OptimizeEssentialGraph(orbfe_context *ctx, std::vector<float> &vTcw, std::vector<float> &vOw, int32_t nLoopKF,
                                                       const std::vector<EssentialEdge> &vEdges, const std::vector<double> &vCorrected,
                                                       const std::vector<uint8_t> &vbCorrected, const std::vector<double> &vNonCorrected,
                                                       const std::vector<uint8_t> &vbNonCorrected, std::vector<float> &vWorldPos,
                                                       const std::vector<int32_t> &vPointRef, const std::vector<uint8_t> &vbPointValid, bool bFixScale,
                                                       int nIterations = 20, double dInitialLambda = (double)(float)1.0e-16)
    {
        const size_t K = vTcw.size() / 16, E = vEdges.size(), N = vPointRef.size();
        if (vTcw.size() != 16 * K || K == 0 || vWorldPos.size() != 3 * N || vbPointValid.size() != N || (!vCorrected.empty() && (vCorrected.size() != 8 * K || vbCorrected.size() != K)) ||
            (vCorrected.empty() != vbCorrected.empty()) || (!vNonCorrected.empty() && (vNonCorrected.size() != 8 * K || vbNonCorrected.size() != K)) ||
            (vNonCorrected.empty() != vbNonCorrected.empty()))
            throw std::invalid_argument("Optimizer::OptimizeEssentialGraph: arrays differ in length");
        std::vector<int32_t> ei(E), ej(E);
        std::vector<uint8_t> ek(E);
        for (size_t e = 0; e < E; e++) { ei[e] = vEdges[e].i; ej[e] = vEdges[e].j; ek[e] = vEdges[e].kind; }
        vOw.resize(3 * K);
        EssentialGraphResult r;
        r.vEdgeCode.assign(E, 0);
        r.vPointCode.assign(N, 0);
        r.vSim3.assign(8 * K, 0.0);
        r.status = 0;
        const int rc = orbfe_optimize_essential_graph(ctx, (int)K, nLoopKF, vTcw.data(), vCorrected.empty() ? nullptr : vCorrected.data(),
                                                      vCorrected.empty() ? nullptr : vbCorrected.data(), vNonCorrected.empty() ? nullptr : vNonCorrected.data(),
                                                      vNonCorrected.empty() ? nullptr : vbNonCorrected.data(), ei.data(), ej.data(), ek.data(), (int)E, nIterations,
                                                      bFixScale ? 1 : 0, dInitialLambda, vWorldPos.data(), vPointRef.data(), vbPointValid.data(), (int)N, vOw.data(),
                                                      r.vEdgeCode.data(), r.vPointCode.data(), r.vSim3.data(), &r.info, &r.status);
        if (rc != ORBFE_OK) throw std::runtime_error(std::string("orbfe: ") + orbfe_last_error(ctx));
        return r;
    }
};

} // namespace ORB_SLAM2
