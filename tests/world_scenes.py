"""One small world per chain of INTEGRATION.md ("Relocalization", "ComputeSim3"), consistent for bag of words, geometry and
descriptors at once, and the chains' models: every stage's EXISTING model, each fed the previous stage's output.  No arithmetic of its
own but one scaling of a point along its viewing ray (_candidate, `deep`): the frame is the oracle's extraction (which the extraction kernels equal bit for bit, tests/test_gpu_parity.py), map points are
tests/test_matchers.py::_frame_scene's, the vocabulary tests/test_bow_device.py::_vocab, the stage models tests/test_bow_device_batch.py::_search,
tests/pnp_solver_model.py, tests/test_reloc_projection_device.py::_expect, oracle.pose_optimization, the orc_search_by_bow_kf oracle,
tests/sim3_solver_model.py, tests/matcher_census.py::oracle_run and tests/sim3_opt_model.py.

tests/test_world_scenes.py shows on the CPU that these worlds decide something at every stage and stay clear of every gate;
tests/test_chain_relocalization.py and tests/test_chain_compute_sim3.py run the chains on the device and verify every stage with the
stage functions below, fed the DEVICE's snapshot from before that stage.

Seeds, and what they give (printed by tests/test_world_scenes.py):
  relocalisation  frame synth.stereo_pair seed 701 (1505 keypoints, 531 stereo), map points _frame_scene seed 701; candidates seeds 31 - 34
                  (340, 380, 150, 400 slots; 162, 169, 92, 171 nodes): BoW matches 175 201 2 0, PnP events 26 2 0 0 (27 3 0 0 with
                  distortion set), the projection stages add 136 13 and 91 16 (136 21 and 83 19) for candidates 0 and 1.
  loop            matcher_census.build("among") (500 and 242 keypoints); draw rows seeds 41 - 43, the displaced third of candidate 1 seed 42,
                  the 12 good points of candidate 2 seed 43: pairs 42 42 12, RANSAC events 41 13 0, OptimizeSim3 keeps 53 and 39.
"""
import numpy as np

from oracle import oracle as O
from tests import pnp_solver_model as PM
from tests import pnp_solver_scenes as PS
from tests import test_bow as TB
from tests import test_matchers as TM

W, H, NL = TM.W, TM.H, TM.NL
BOW_LEVEL, BOW_RATIO, BOW_ORI = 4, 0.75, True                      # Relocalization's matcher(0.75, true), src/Tracking.cc:1455
PNP = dict(min_inliers=PS.MIN_INLIERS, max_its=PS.MAX_ITS, epsilon=PS.EPSILON, n_iterations=PS.ITERATE, th2=PS.TH2)   # :1488, iterate(5)
STAGES = ((10.0, 100), (3.0, 64))                                  # SearchByProjection at :1552 and :1566; both check the rotation
DIST = [-0.28, 0.07, 2e-4, 1e-5, 0.0]                              # tests/test_reloc_projection_device.py's coefficients
FRAME_SEED = 701
ERR_INVALID = -1
_CACHE = {}
_TABLES = {}


def vocab():
    from tests import test_bow_device as TD
    return TD._vocab()


def its_table(capacity):
    """PnPRansacIterationTable(capacity, 0.99, 10, 300, 0.5): Tracking's parameters."""
    if capacity not in _TABLES:
        _TABLES[capacity] = PM.its_table(capacity, PS.PROB, PNP["min_inliers"], PNP["max_its"], PNP["epsilon"])
    return _TABLES[capacity]


def _frame(distorted):
    """The oracle's extraction of the stereo pair at nfeatures = 1500: what enqueue_stereo leaves in slot 0."""
    from orbslam2_amd import synth
    left, right = synth.stereo_pair(W, H, seed=FRAME_SEED)
    exl, exr = O.Extractor(nfeatures=1500), O.Extractor(nfeatures=1500)
    k, d = exl.extract(left)
    kr, dr = exr.extract(right)
    ur = O.stereo_matches(exl, exr, k, d, kr, dr, TM.BF, TM.FX)[0]
    kun, bounds = k, (0.0, float(W), 0.0, float(H))
    if distorted:
        und = O.undistort_points(np.stack([k["x"], k["y"]], 1), TM.FX, TM.FY, TM.CX, TM.CY, DIST)
        kun = k.copy(); kun["x"], kun["y"] = und[:, 0], und[:, 1]
        bounds = tuple(float(b) for b in O.image_bounds(W, H, TM.FX, TM.FY, TM.CX, TM.CY, DIST))
    sf = exl.scale_factors()
    return dict(images=np.stack([left, right]).astype(np.uint8), k_raw=k, k=kun, d=d, ur=ur, bounds=bounds, sf=sf, grid=O.Grid(kun, *bounds),
                sigma2=exl.sigma2(), inv_sigma2=exl.inv_sigma2())


def _candidate(fr, s, seed, n, flip=0.02, wrong=0.0, deep=0.0, n_copy=None, pvalid=0.9):
    """A keyframe of n slots: n_copy (default all) are a permuted subset of the frame's keypoints -- descriptor with `flip` of its bits
    flipped, angle jittered, pos the keypoint's true map point -- the rest noise (TB._descs, a position somewhere).  wrong: that
    share of the copied slots gets the position of ANOTHER keypoint's point (a gross outlier).  deep: that share of the copied slots
    of STEREO keypoints carries its point at 1.5 times its depth on the keypoint's viewing ray (the true pose is the identity): PnP,
    which reads no mvuRight, keeps such a point, the pose optimisation's stereo edge flags it, the projection stage behind it clears
    it, and the 3 / 64 stage -- whose sFound no longer holds it -- finds it again.  max / min distance as
    tests/test_reloc_projection_device.py::_real_frame forms them."""
    rng = np.random.default_rng(seed)
    nk = len(fr["k"])
    n_copy = n if n_copy is None else n_copy
    perm = rng.permutation(nk)[:n_copy]
    d = np.concatenate([TB._descs(seed + 100, 0, base=fr["d"][perm], flip=flip), TB._descs(seed + 200, n - n_copy)])
    ang = np.concatenate([(fr["k"]["angle"][perm] + rng.normal(0, 4, n_copy)) % 360, rng.uniform(0, 360, n - n_copy)]).astype(np.float32)
    ang[ang >= 360] = 0
    src = np.concatenate([perm, rng.permutation(nk)[:n - n_copy]])         # the keypoint whose point a slot carries
    bad = np.zeros(n, bool)
    bad[:n_copy] = rng.random(n_copy) < wrong
    src = np.where(bad, (src + 1 + rng.integers(0, nk - 1, n)) % nk, src)
    far = np.zeros(n, bool)
    far[:n_copy] = (rng.random(n_copy) < deep) & (fr["ur"][perm] > 0) & ~bad[:n_copy]
    pos = np.where(far[:, None], s["pos"][src] * np.float32(1.5), s["pos"][src])
    octave = np.concatenate([fr["k"]["octave"][perm], rng.integers(0, NL, n - n_copy)])
    dist0 = np.linalg.norm(pos, axis=1).astype(np.float32)
    max_d = (dist0 * fr["sf"][octave]).astype(np.float32)
    return dict(d=np.ascontiguousarray(d), ang=ang, pos=np.ascontiguousarray(pos, np.float32), valid=(rng.random(n) < pvalid).astype(np.int32),
                max_d=max_d, min_d=(max_d / fr["sf"][NL - 1]).astype(np.float32), of=perm, wrong=bad, far=far, draws=PS.draws(seed + 1000, PNP["max_its"]), seed=seed)


def reloc_world(distorted=False):
    """The relocalisation world: the frame, its true pose (the identity: _frame_scene back-projects the keypoints there), K = 4
    candidates with their feature vectors.  max_kf_nnodes bounds candidates 0 - 2; candidate 3 has more nodes and is refused."""
    key = ("reloc", distorted)
    if key in _CACHE:
        return _CACHE[key]
    fr = _frame(distorted)
    s = TM._frame_scene(fr["k"], fr["d"], fr["ur"], FRAME_SEED, all_points=True)        # one map point per keypoint
    cands = [_candidate(fr, s, 31, 340, deep=0.4), _candidate(fr, s, 32, 380, wrong=0.4, deep=0.7), _candidate(fr, s, 33, 150, n_copy=6, pvalid=1.0),
             _candidate(fr, s, 34, 400)]
    L, v = TB._oracle_voc(vocab())
    per, fbow, f_fv = TB._oracle_transform(L, v, fr["d"], BOW_LEVEL)
    for c in cands:
        c["fv"] = TB._oracle_transform(L, v, c["d"], BOW_LEVEL)[2]
    L.orc_vocab_destroy(v)
    w = dict(fr=fr, truth=np.eye(4, dtype=np.float32), cands=cands, per=per, fbow=fbow, f_fv=f_fv, max_kf_nnodes=max(len(c["fv"][0]) for c in cands[:3]),
             max_kf_n=max(len(c["valid"]) for c in cands), distorted=distorted)
    _CACHE[key] = w
    return w


# ------------------------------------------------------------------ the stages of Relocalization, each an existing model
def stage_bow(w, c, refused=None):
    """Row c of orbfe_enqueue_search_by_bow_batch: (f_match[nk], nmatches, status, has[nk]).  A record with nnodes above the bound is
    searched as a keyframe without nodes (include/orbfe.h)."""
    from tests import test_bow_device_batch as TBB
    fr, kf = w["fr"], w["cands"][c]
    nk = len(fr["k"])
    refused = len(kf["fv"][0]) > w["max_kf_nnodes"] if refused is None else refused
    if refused:
        return np.full(nk, -1, np.int32), 0, ERR_INVALID, np.zeros(nk, np.uint8)
    m, nm = TBB._search(O.lib(), kf, w["f_fv"], fr["d"], np.ascontiguousarray(fr["k_raw"]["angle"]), BOW_RATIO, BOW_ORI)
    return m.astype(np.int32), int(nm), 0, (m >= 0).astype(np.uint8)


def pnp_scene(w, c, f_match):
    """Candidate c with the row f_match as tests/pnp_solver_model.py takes a scene (capacity = the frame's keypoint count)."""
    fr, kf = w["fr"], w["cands"][c]
    nk = len(fr["k"])
    return dict(keys=fr["k"], f_match=np.asarray(f_match, np.int32), pos=kf["pos"], valid=kf["valid"], draws=kf["draws"], capacity=nk, sigma2=fr["sigma2"],
                cam=(TM.FX, TM.FY, TM.CX, TM.CY), its_for_n=its_table(nk), **PNP)


def stage_pnp(w, c, f_match):
    return PM.run(pnp_scene(w, c, f_match))


def pick(rows):
    """What the host decides on the fetched rows: the first event, or (a candidate without one) event 0, which select refuses."""
    return (PM.EVENT, int(rows["events"][0]) if rows["n_events"] > 0 else 0)


def stage_select(w, rows, which, k, capacity, untouched_point, untouched_has):
    """(Tcw[16], cur_point[capacity], has[capacity], status) of orbfe_enqueue_pnp_ransac_select."""
    return PM.select_rows(rows, which, k, len(w["fr"]["k"]), capacity, untouched_point, untouched_has)


def stage_pose(w, T, has, Xw, outlier):
    """orbfe_enqueue_pose_optimization on one row: (Tcw 4x4, outlier[nk], n_inliers, the oracle's trace).  Xw rows of keypoints without
    a point are never read: they are zeroed here so that a poison there cannot reach the oracle either."""
    fr = w["fr"]
    nk = len(fr["k"])
    has = np.ascontiguousarray(has[:nk], np.uint8)
    X = np.where(has[:, None] != 0, np.asarray(Xw, np.float32).reshape(-1, 3)[:nk], np.float32(0))
    T2, out, n = O.pose_optimization(np.asarray(T, np.float32).reshape(4, 4), fr["k"], fr["ur"], has, X, fr["inv_sigma2"], TM.FX, TM.FY, TM.CX, TM.CY, TM.BF,
                                     outlier=np.asarray(outlier[:nk], np.uint8))
    return T2, out, int(n), O.pose_trace()


def stage_projection(w, c, T, cur_point, outlier, stage, n=None):
    """Row c of orbfe_enqueue_search_by_projection_kf_batch at STAGES[stage] (exclude_held = 1, rotation check on): the dict of
    tests/test_reloc_projection_device.py::_expect.  outlier is None at the second stage (src/Tracking.cc:1566)."""
    from tests import test_reloc_projection_device as TR
    fr, kf = w["fr"], w["cands"][c]
    nk = len(fr["k"])
    th, od = STAGES[stage]
    rec = dict(T=np.ascontiguousarray(np.asarray(T, np.float32).reshape(4, 4)), pos=kf["pos"], desc=kf["d"], valid=kf["valid"], angle=kf["ang"], max_d=kf["max_d"],
               min_d=kf["min_d"], th=th, od=od)
    return TR._expect(fr, rec, np.asarray(cur_point[:nk], np.int32), None if outlier is None else np.asarray(outlier[:nk], np.uint8), 1, True)


def held_Xw(w, c, cur_point, Xw_before):
    """The d_Xw row after a matcher call: pos of the held point for every held keypoint, rows without a point as they were."""
    nk = len(w["fr"]["k"])
    X = np.array(Xw_before, np.float32).reshape(-1, 3).copy()
    cp = np.asarray(cur_point[:nk])
    X[:nk][cp >= 0] = w["cands"][c]["pos"][cp[cp >= 0]]
    return X


def model_chain_reloc(w):
    """The whole chain on the models alone, per candidate: a list of dicts with every stage's output."""
    key = ("chain", w["distorted"])
    if key in _CACHE:
        return _CACHE[key]
    nk = len(w["fr"]["k"])
    out = []
    for c in range(len(w["cands"])):
        r = {}
        r["f_match"], r["nm"], r["bow_status"], has = stage_bow(w, c)
        Xw = held_Xw(w, c, r["f_match"], np.full((nk, 3), np.nan, np.float32))
        r["pnp"] = stage_pnp(w, c, r["f_match"])
        r["pick"] = pick(r["pnp"])
        T, cur, has, r["select_status"] = stage_select(w, r["pnp"], *r["pick"], nk, -1, 0)
        r["select"] = (T.copy(), cur.copy(), has.copy())
        outl = np.zeros(nk, np.uint8)
        r["pose"], r["proj"] = [], []
        for stage in range(3):
            T, outl, n_in, trace = stage_pose(w, T, has, Xw, outl)
            r["pose"].append(dict(T=T.copy(), outlier=outl.copy(), n_inliers=n_in, trace=trace, has=has.copy()))
            if stage == 2:
                break
            e = stage_projection(w, c, T, cur, outl if stage == 0 else None, stage)
            e["cur_before"] = cur.copy()
            cur, has = e["cur_point"], e["has"]
            Xw = held_Xw(w, c, cur, Xw)
            r["proj"].append(e)
        out.append(r)
    _CACHE[key] = out
    return out


# ====================================================================== the loop world: LoopClosing::ComputeSim3
SIM3 = dict(min_inliers=20, max_its=300, fix_scale=0)               # src/LoopClosing.cc:298, include/Sim3Solver.h:50
SIM3_TH, OPT_TH2, LOOP_TH = 7.5, 10.0, 10.0                        # SearchBySim3 (:359), OptimizeSim3 (:362), SearchByProjection (:411)
LOOP_BOW_LEVEL = 1                                                  # the ten nodes below the root: random descriptors 18 bits apart seldom share a deeper one
LOOP_SEEDS = (41, 42, 43)                                           # the draw rows; 42 and 43 also build candidates 1 and 2


def loop_world():
    """matcher_census.build("among"): KF1 (mpCurrentKF) is the scene's first keyframe (one keypoint per map point, at T_last), candidate 0
    its second (T_cur).  Candidate 1 is a copy in which a third of the slots that SearchByBoW pairs hold ANOTHER slot's point (displaced);
    candidate 2 a copy whose map points are all bad but 12, so fewer than 20 pairs are accepted.  Feature vectors: _oracle_transform."""
    if "loop" in _CACHE:
        return _CACHE["loop"]
    from tests import bow_kf_scenes as BK
    from tests import matcher_census as MC
    from tests import sim3_solver_model as SM
    from tests import sim3_solver_scenes as SS
    s = MC.build("among")
    n1, n2 = len(s["k1"]), len(s["k"])
    L, v = TB._oracle_voc(vocab())
    fv = lambda d: TB._oracle_transform(L, v, np.ascontiguousarray(d), LOOP_BOW_LEVEL)[2]
    kf1 = BK._kf(fv(s["d1"]), s["pts1"][4], s["d1"], s["k1"]["angle"].copy())
    fv2 = fv(s["d"])
    L.orc_vocab_destroy(v)
    pos2, mx2, mn2, d2, valid2 = s["pts2"]
    src = s["src"]
    normal2 = np.zeros((n2, 3), np.float32); normal2[src >= 0] = s["normal"][src[src >= 0]]
    base = dict(k=np.ascontiguousarray(s["k"]), d=np.ascontiguousarray(d2), ang=s["k"]["angle"].copy(), fv=fv2, pos=np.ascontiguousarray(pos2, np.float32).reshape(n2, 3),
                normal=normal2, max_d=mx2, min_d=mn2, valid=np.asarray(valid2, np.int32), T2w=np.ascontiguousarray(s["T_cur"], np.float32)[:3])
    first = BK.oracle(kf1, BK._kf(fv2, base["valid"], base["d"], base["ang"]), BOW_RATIO, BOW_ORI)[0]
    paired = first[first >= 0]
    rng = np.random.default_rng(LOOP_SEEDS[1])
    moved = np.sort(rng.choice(paired, len(paired) // 3, replace=False))
    c1 = dict(base, pos=base["pos"].copy(), moved=moved)
    c1["pos"][moved] = base["pos"][np.roll(moved, 1)]                # the point of another paired slot: metres away
    rng = np.random.default_rng(LOOP_SEEDS[2])
    few = np.zeros(n2, np.int32); few[rng.choice(paired, 12, replace=False)] = 1
    cands = [dict(base), c1, dict(base, valid=few)]
    for i, c in enumerate(cands):
        c["draws"] = SS.draws(LOOP_SEEDS[i], SIM3["max_its"])
        c["bow"] = BK._kf(c["fv"], c["valid"], c["d"], c["ang"])
    w = dict(s=s, n1=n1, n2=n2, kf1=kf1, keys1=np.ascontiguousarray(s["k1"]), pos1=np.ascontiguousarray(s["pts1"][0], np.float32).reshape(n1, 3),
             valid1=np.asarray(s["pts1"][4], np.int32), T1w=np.ascontiguousarray(s["T_last"], np.float32)[:3], cands=cands, max_kf_n=max(n1, n2),
             its_for_n=SM.its_table(n1, SS.PROB, SIM3["min_inliers"], SIM3["max_its"]), sigma2=SS.SIGMA2)
    _CACHE["loop"] = w
    return w


def loop_bow(w, i):
    """Row i of orbfe_enqueue_search_by_bow_kf_batch: (match12[n1], pairs[2 * count], count)."""
    from tests import bow_kf_scenes as BK
    m, n = BK.oracle(w["kf1"], w["cands"][i]["bow"], BOW_RATIO, BOW_ORI)
    return m, BK.pairs_of(m), int(n)


def loop_ransac(w, i, pairs):
    """Row i of orbfe_enqueue_sim3_ransac_batch on the pairs (count x 2) where the BoW batch left them; max_pairs = n1."""
    from tests import sim3_opt_scenes as OS
    from tests import sim3_solver_model as SM
    c = w["cands"][i]
    return SM.run(dict(keys1=w["keys1"], pos1=w["pos1"], valid1=w["valid1"], T1w=w["T1w"], keys2=c["k"], pos2=c["pos"], valid2=c["valid"], T2w=c["T2w"],
                       pairs=np.asarray(pairs, np.int32).reshape(-1, 2), draws=c["draws"], max_pairs=w["n1"], max_kf_n=w["max_kf_n"], sigma2=w["sigma2"], cam=OS.CAM,
                       its_for_n=w["its_for_n"], **SIM3))


def loop_select(w, i, rows, k):
    from tests import sim3_solver_model as SM
    return SM.select_rows(rows, k, w["n1"], w["valid1"], w["cands"][i]["valid"])


def loop_by_sim3(w, i, hyp, v1, v2):
    """orbfe_enqueue_search_by_sim3 with hypothesis `hyp` and the round's valid arrays: (match12, n_found)."""
    from tests import matcher_census as MC
    s, c = w["s"], w["cands"][i]
    p1, p2 = s["pts1"], s["pts2"]
    run = dict(s, pts1=(p1[0], p1[1], p1[2], p1[3], np.asarray(v1, np.int32)), pts2=(c["pos"], c["max_d"], c["min_d"], c["d"], np.asarray(v2, np.int32)[:w["n2"]]),
               s12=np.float32(hyp["s12"]), R12=np.asarray(hyp["R12"], np.float32).reshape(3, 3), t12=np.asarray(hyp["t12"], np.float32))
    return MC.oracle_run("by_sim3", run, (SIM3_TH,))


def loop_optimize(w, i, hyp, prior, match12):
    """orbfe_enqueue_optimize_sim3 behind it: the dict of tests/sim3_opt_model.py::optimize_sim3."""
    from tests import sim3_opt_model as OM
    from tests import sim3_opt_scenes as OS
    c = w["cands"][i]
    return OM.optimize_sim3(w["keys1"], w["T1w"], w["pos1"], w["valid1"], c["k"], c["T2w"], c["pos"], c["valid"], hyp["s12"], hyp["R12"], hyp["t12"], OPT_TH2,
                            SIM3["fix_scale"], match12, OS.CAM, OS.INV_SIGMA2, OS.NLEVELS, prior12=prior)


def loop_scw(w, i, S12):
    """mg2oScw = gScm * gSmw of src/LoopClosing.cc:385-411, composed on the host from the fetched S12 (qx qy qz qw tx ty tz s) and the
    candidate's pose, as the 3 x 4 [sR | t] the projection call takes."""
    from tests import sim3_opt_model as OM
    T2 = w["cands"][i]["T2w"].astype(np.float64)
    return np.ascontiguousarray(OM.sim3_matrix(OM.sim3_mul(OM.unpack(S12), OM.sim3(T2[:, :3], T2[:, 3], 1.0)))[:3], np.float32)


def loop_projection_inputs(w, i, match12):
    """(kf_matched[n1], pt_valid[n2]) from the optimiser's surviving matches (:362-373, src/ORBmatcher.cc:301-302)."""
    m = np.asarray(match12)
    found = np.zeros(w["n2"], bool)
    found[m[m >= 0]] = True
    return (m >= 0).astype(np.uint8), ((w["cands"][i]["valid"] != 0) & ~found).astype(np.int32)


def loop_projection(w, i, Scw, kf_matched, pt_valid):
    """orbfe_enqueue_search_by_projection_sim3 of the candidate's map points into KF1: (pt_match[n2], count)."""
    from tests import matcher_census as MC
    s, c = w["s"], w["cands"][i]
    run = dict(s, k=w["keys1"], d=s["d1"], Scw=Scw, pos=c["pos"], normal=c["normal"], max_d=c["max_d"], min_d=c["min_d"], desc=c["d"],
               valid=np.asarray(pt_valid, np.int32), kf_matched=np.asarray(kf_matched, np.uint8))
    return MC.oracle_run("sim3_projection", run, (LOOP_TH,))


def model_chain_loop(w):
    """The whole chain on the models alone, per candidate."""
    if "loop_chain" in _CACHE:
        return _CACHE["loop_chain"]
    out = []
    for i in range(len(w["cands"])):
        r = {}
        r["match12"], r["pairs"], r["nm"] = loop_bow(w, i)
        r["ransac"] = rows = loop_ransac(w, i, r["pairs"][:2 * r["nm"]])
        if rows["n_events"] > 0:
            k = r["k"] = int(rows["events"][0])
            hyp = rows["hyp"][k]
            r["select"] = prior, v1, v2 = loop_select(w, i, rows, k)
            r["by_sim3"] = loop_by_sim3(w, i, hyp, v1, v2)
            r["opt"] = loop_optimize(w, i, hyp, prior, r["by_sim3"][0])
            r["Scw"] = loop_scw(w, i, r["opt"]["S12"])
            r["proj_in"] = loop_projection_inputs(w, i, r["opt"]["match12"])
            r["proj"] = loop_projection(w, i, r["Scw"], *r["proj_in"])
        out.append(r)
    _CACHE["loop_chain"] = out
    return out
