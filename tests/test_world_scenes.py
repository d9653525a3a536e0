"""The worlds of tests/world_scenes.py on the models alone (no GPU): every stage of both chains decides something and stays clear of
every gate, so the GPU comparisons of tests/test_chain_relocalization.py and tests/test_chain_compute_sim3.py can be exact and leave
nothing out.  The per-stage counts are printed (pytest -s); the seeds that give them are stated in tests/world_scenes.py.

Relocalisation world, as printed (plain / with distortion set):
  BoW matches 175 201 2 0 (status 0 0 0 -1); PnP correspondences 175 201 2 0, iterations 35 35 0 0, events 26 2 0 0 / 27 3 0 0;
  candidate 0: pose keeps 162 289 289 / 154 274 274, the projection stages add 136 13 / 136 21, 13 / 21 entries cleared by outlier flags;
  candidate 1: pose keeps 106 185 187 / 103 176 178, the projection stages add 91 16 / 83 19, 14 / 17 entries cleared."""
import numpy as np
import pytest

from tests import world_scenes as WS


@pytest.mark.parametrize("distorted", [False, True])
def test_the_relocalisation_world_decides_every_stage(distorted):
    w = WS.reloc_world(distorted)
    ch = WS.model_chain_reloc(w)
    nk = len(w["fr"]["k"])
    assert len(w["cands"]) == 4 and all(150 <= len(c["valid"]) <= 400 for c in w["cands"]) and 1000 < nk <= 1500 + 64 * 8
    assert len(w["cands"][3]["fv"][0]) > w["max_kf_nnodes"] >= max(len(c["fv"][0]) for c in w["cands"][:3])
    print("\nrelocalisation world%s: %d keypoints, %d stereo; nodes %s against the bound %d" % (
        " (distortion set)" if distorted else "", nk, int((w["fr"]["ur"] > 0).sum()), [len(c["fv"][0]) for c in w["cands"]], w["max_kf_nnodes"]))
    for c, r in enumerate(ch):
        p = r["pnp"]
        print("candidate %d: BoW %3d matches (status %2d); PnP N %3d, %2d iterations, %2d events, pick %s -> select status %2d, %3d points held" % (
            c, r["nm"], r["bow_status"], p["n_corr"], p["n_its"], p["n_events"], r["pick"], r["select_status"], int((r["select"][1] >= 0).sum())))
        for s in range(3):
            q = r["pose"][s]
            print("    pose %d: %3d points, %3d inliers, min margin %.3g" % (s, int(q["has"].sum()), q["n_inliers"], q["trace"]["min_margin"]))
            if s < 2:
                e = r["proj"][s]
                cleared = int(((e["cur_before"] >= 0) & (q["outlier"] != 0)).sum()) if s == 0 else 0
                print("    projection %s: %3d new matches, %2d entries cleared by outlier flags" % (WS.STAGES[s], e["nm"], cleared))
    # BoW
    assert ch[0]["nm"] >= 15 and ch[1]["nm"] >= 15 and ch[2]["nm"] < 15 and ch[2]["nm"] < WS.PNP["min_inliers"]
    assert ch[3]["nm"] == 0 and ch[3]["bow_status"] == WS.ERR_INVALID and [r["bow_status"] for r in ch[:3]] == [0, 0, 0]
    # PnP: the bounds of tests/test_pnp_solver_model.py against the truth
    for c in (0, 1):
        assert ch[c]["pnp"]["n_events"] >= 1 and ch[c]["pnp"]["status"] == 0 and ch[c]["select_status"] == 0
    T = ch[0]["select"][0].reshape(4, 4)
    assert np.abs(T[:3, :3] - w["truth"][:3, :3]).max() < 0.02 and np.abs(T[:3, 3] - w["truth"][:3, 3]).max() < 0.2
    for c in (2, 3):
        assert ch[c]["pnp"]["n_its"] == 0 and ch[c]["select_status"] == WS.ERR_INVALID
        assert np.array_equal(ch[c]["select"][0].reshape(4, 4), np.eye(4, dtype=np.float32)) and not ch[c]["select"][2].any()
    assert any(c["wrong"][r["f_match"][r["f_match"] >= 0]].any() for c, r in zip(w["cands"][1:2], ch[1:2]))    # PnP has outliers to reject
    # the refinement
    cleared_total = 0
    for c in (0, 1):
        r = ch[c]
        assert r["proj"][0]["nm"] >= 10 and r["proj"][1]["nm"] >= 10, (c, r["proj"][0]["nm"], r["proj"][1]["nm"])
        assert all(e["status"] == 0 for e in r["proj"])
        cleared_total += int(((r["proj"][0]["cur_before"] >= 0) & (r["pose"][0]["outlier"] != 0)).sum())
        found10 = np.zeros(len(w["cands"][c]["valid"]), bool); found3 = found10.copy()
        cb10, cb3 = r["proj"][0]["cur_before"], r["proj"][1]["cur_before"]
        found10[cb10[cb10 >= 0]] = True; found3[cb3[cb3 >= 0]] = True
        assert (found3 & ~found10).any() and (found10 & ~found3).any()     # sFound changes meaning between the two stages, both ways
        for q in r["pose"]:
            assert q["trace"]["min_margin"] >= 1e-4, (c, q["trace"]["min_margin"])   # the bound of tests/test_pose_census.py
    assert cleared_total >= 1
    assert all(q["n_inliers"] > 50 for q in ch[0]["pose"])
    # candidates 2 and 3 run every stage from the identity: no point at the first pose stage, a projection row behind it
    for c in (2, 3):
        assert ch[c]["pose"][0]["n_inliers"] == 0 and np.array_equal(ch[c]["pose"][0]["T"], np.eye(4, dtype=np.float32))


def test_the_loop_world_decides_every_stage():
    """As printed: 500 and 242 keypoints, 10 nodes each; pairs 42 42 12; RANSAC iterations 41 41 0, events 41 13 0; candidate 0: hypothesis
    0 with 42 inliers, SearchBySim3 adds 11, OptimizeSim3 keeps 53 of 53 (margin 0.585), the projection adds 6; candidate 1: hypothesis 1
    with 28 inliers, 11 added, 39 of 39 kept (margin 0.792), the projection adds 6."""
    from tests import sim3_opt_scenes as OS
    w = WS.loop_world()
    ch = WS.model_chain_loop(w)
    assert len(w["cands"]) == 3 and w["n1"] != w["n2"]
    print("\nloop world: %d and %d keypoints, nodes %d and %s" % (w["n1"], w["n2"], len(w["kf1"]["fv"][0]), [len(c["fv"][0]) for c in w["cands"]]))
    for i, r in enumerate(ch):
        q = r["ransac"]
        print("candidate %d: %2d pairs, N %2d, %2d iterations, %2d events (status %d)" % (i, r["nm"], q["n_corr"], q["n_its"], q["n_events"], q["status"]))
        if "k" in r:
            print("    hypothesis %d: %d RANSAC inliers, SearchBySim3 adds %d, OptimizeSim3 keeps %d of %d (margin %.3g, iterations %s), the projection adds %d "
                  "(%d keypoints matched on entry, %d valid points)" % (r["k"], q["hyp"]["n_inliers"][r["k"]], r["by_sim3"][1], r["opt"]["n_inliers"], r["opt"]["n_corr"],
                                                                        OS.margin(r["opt"], WS.OPT_TH2), r["opt"]["iterations"], r["proj"][1], int(r["proj_in"][0].sum()),
                                                                        int(r["proj_in"][1].sum())))
    for i in (0, 1):
        r = ch[i]
        assert r["nm"] >= 20 and r["ransac"]["n_events"] >= 1 and r["ransac"]["status"] == 0, i
        assert r["by_sim3"][1] > 0 and r["opt"]["status"] == 0 and r["opt"]["n_inliers"] >= 20 and r["proj"][1] > 0, i
        assert OS.margin(r["opt"], WS.OPT_TH2) > 0.01, i                 # the rule of tests/test_sim3_opt_model.py
        assert (r["select"][0] >= 0).sum() == r["ransac"]["hyp"]["n_inliers"][r["k"]]
    moved = w["cands"][1]["moved"]
    paired1 = ch[1]["match12"][ch[1]["match12"] >= 0]
    assert 3 * len(moved) >= len(paired1) - 2 and np.isin(moved, paired1).all()       # a third of the matched points is displaced ...
    assert not np.isin(moved, ch[1]["select"][0]).any()                               # ... and the chosen hypothesis rejects every one of them
    assert ch[2]["nm"] < 20 and ch[2]["ransac"]["n_its"] == 0 and ch[2]["ransac"]["n_events"] == 0
    assert np.array_equal(ch[0]["match12"], ch[1]["match12"]) and not np.array_equal(ch[0]["ransac"]["bits"], ch[1]["ransac"]["bits"])
