"""Tracking::Relocalization end to end on one stream, as INTEGRATION.md tells an integrator to queue it: enqueue_stereo -> compute_bow
-> search_by_bow_batch -> pnp_ransac_batch (its records point INTO the d_f_match rows) -> one download of the events -> select per
candidate -> pose -> projection batch (10, 100) -> pose -> projection batch (3, 64, no outlier array) -> pose, the last six without
a host step.  The world is tests/world_scenes.py::reloc_world (checked on the CPU by tests/test_world_scenes.py): candidates 0 and 1
are live, candidate 2 is one the BoW stage would have discarded (2 matches, n_its = 0, select gives ORBFE_ERR_INVALID and the
identity), candidate 3 a record the BoW batch refuses; all four run every stage.

What each test pins is the SEAMS -- one call's HBM rows are the next call's input and never pass through the host:
  * where no contract promises a value the caller's arrays hold poison (d_f_match and cur_point at and beyond the slot's count:
    device_arrays.BEYOND; every d_Xw row: NaN until a matcher writes it; mvbOutlier beyond the count: 1); has_point rows are zero at
    and beyond the count, the caller's duty.  The poison must reach no result and must still be there afterwards;
  * after every stage the rows are copied on the same stream (snapshots), and every stage is verified on its own: its existing model
    (tests/world_scenes.py::stage_*) is fed the DEVICE's snapshot from before that stage.  Integer and bit results are exact and
    nothing is left out; a pose is compared with oracle.pose_optimization within POSE_ATOL of tests/test_pose.py, its outlier flags
    and inlier count exactly.  So a pose difference of 1e-6 cannot flip a window downstream of the comparison;
  * the chain runs in a context that has made no other call (every lazy state and grow-only scratch is created mid-chain), again in the
    same context, with distortion set, and with candidates 0 and 1 alone (bit-identical rows).

Largest |pose - oracle| over all candidates and both runs, as printed on the MI355X: 0, 0, 0 at the three pose
stages of the plain world; 0, 5.6e-17, 3.0e-14 with distortion set.
"""
import numpy as np
import pytest

from orbslam2_amd import bow as B
from tests import pnp_solver_model as PM
from tests import world_scenes as WS
from tests.device_arrays import BEYOND, UNTOUCHED, Guarded, context, device_buffers, raw, upload, upload_records

PAD = 64
STAGE_ROWS = ("T", "cur", "has", "Xw", "outlier")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


class _Chain:
    """The arrays of one relocalisation in HBM -- inputs between PAD readable entries, outputs between guard rows, poisoned as the module
    docstring says -- and the queue of INTEGRATION.md.  ids: the world's candidates that take part."""

    def __init__(self, api, ctx, st, w, ids):
        from tests import test_bow_device as TD
        from tests import test_pnp_ransac_device as TP
        self.api, self.ctx, self.st, self.w, self.ids = api, ctx, st, w, list(ids)
        self.K, self.cap, self.nk = len(self.ids), ctx.capacity, len(w["fr"]["k"])
        K, cap, nk, mi = self.K, self.cap, self.nk, WS.PNP["max_its"]
        self.words = (cap + 31) // 32
        self.own = []
        up = self._up
        self.d_img = upload(w["fr"]["images"])[0]
        self.fv = TD._Fv(cap)
        bow, pnp, self.dev = [], [], []
        for c in self.ids:
            kf = w["cands"][c]
            d = dict(nodes=up(kf["fv"][0].astype(np.uint32)), off=up(kf["fv"][1].astype(np.int32)), feat=up(kf["fv"][2].astype(np.int32)),
                     valid=up(kf["valid"].astype(np.int32)), desc=up(kf["d"]), angle=up(kf["ang"]), pos=up(kf["pos"]), max_d=up(kf["max_d"]),
                     min_d=up(kf["min_d"]), draws=up(np.ascontiguousarray(kf["draws"], np.uint32).view(np.int32)), n=len(kf["valid"]), nnodes=len(kf["fv"][0]))
            self.dev.append(d)
            bow.append(api.BowKeyframe(d["nodes"], d["off"], d["feat"], d["valid"], d["desc"], d["angle"], d["pos"], d["nnodes"], d["n"]))
        self.d_bow = upload_records(bow)
        # the BoW batch's rows; has_point is zero at and beyond the count because the caller zeroes the rows before the chain
        self.f_match, self.nm, self.bow_status = Guarded.cells(K * cap, BEYOND), Guarded.cells(K), Guarded.cells(K)
        self.has = Guarded(np.zeros(K * cap, np.uint8))
        self.Xw = Guarded(np.full(K * cap * 3, np.nan, np.float32))
        for i, d in enumerate(self.dev):
            r = api.PnPCandidate()
            r.f_match, r.pos, r.valid, r.draws, r.n = self.f_match.ptr + 4 * i * cap, d["pos"], d["valid"], d["draws"], d["n"]   # row i where the BoW batch leaves it
            pnp.append(r)
        self.d_pnp = upload_records(pnp)
        self.table = up(WS.its_table(cap))
        f = TP._filled
        self.pnp = dict(n_corr=Guarded(f(K, np.int32)), n_its=Guarded(f(K, np.int32)), corr=Guarded(f((K * cap, 2), np.int32)),
                        hyp=Guarded(f(K * mi, PM.HYP_DTYPE)), bits=Guarded(f((K * mi, self.words), np.uint32)), refined=Guarded(f(K * mi, PM.REFINED_DTYPE)),
                        refined_bits=Guarded(f((K * mi, self.words), np.uint32)), events=Guarded(f(K * mi, np.int32)), n_events=Guarded(f(K, np.int32)),
                        exhausted=Guarded(f(K, np.int32)), status=Guarded(f(K, np.int32)))
        self.T = Guarded(np.full(K * 16, -7.0, np.float32))
        self.cur = Guarded.cells(K * cap, BEYOND)
        self.select_status = Guarded.cells(K)
        outl = np.ones((K, cap), np.uint8); outl[:, :nk] = 0        # mvbOutlier: false for the frame's keypoints, never read or written beyond them
        self.outlier = Guarded(outl.reshape(-1))
        recs = [[], []]
        for stage, (th, od) in enumerate(WS.STAGES):
            for i, d in enumerate(self.dev):
                recs[stage].append(api.RelocCandidate(Tcw=self.T.ptr + 64 * i, pos=d["pos"], desc=d["desc"], valid=d["valid"], angle=d["angle"], max_distance=d["max_d"],
                                                      min_distance=d["min_d"], cur_point=self.cur.ptr + 4 * i * cap,
                                                      outlier=self.outlier.ptr + i * cap if stage == 0 else None, n=d["n"], th=th, orb_dist=od, reserved=0))
        self.d_cands = [upload_records(r) for r in recs]
        self.new = [Guarded.cells(K * cap), Guarded.cells(K * cap)]
        self.nadd, self.proj_status = [Guarded.cells(K), Guarded.cells(K)], [Guarded.cells(K), Guarded.cells(K)]
        self.ngood = [Guarded.cells(K) for _ in range(3)]
        self.d_off = upload(np.arange(K + 1, dtype=np.int32) * cap)[0]
        import torch
        self.keys_rows = torch.zeros(K * cap * 28, dtype=torch.uint8, device="cuda:0")
        self.ur_rows = torch.zeros(K * cap * 4, dtype=torch.uint8, device="cuda:0")
        self.snaps = {}
        torch.cuda.synchronize()                                    # every upload is in place before the first queued call

    def _up(self, a):
        t, p = upload(a, front=PAD, pad=PAD)
        self.own.append(t)
        return p

    def _snap(self, name):
        import torch
        with torch.cuda.stream(self.st):
            self.snaps[name] = {k: getattr(self, k).view.clone() for k in STAGE_ROWS}
            if name == "bow":
                self.snaps[name]["f_match"] = self.f_match.view.clone()

    def _pose(self, stage):
        ctx, cap = self.ctx, self.cap
        ctx._check(ctx.L.orbfe_enqueue_pose_optimization(ctx.h, self.K, self.d_off.data_ptr(), self.keys_rows.data_ptr(), self.ur_rows.data_ptr(), self.has.ptr,
                                                         self.Xw.ptr, self.T.ptr, self.outlier.ptr, self.ngood[stage].ptr, cap, self.st.cuda_stream))
        self._snap("pose%d" % stage)

    def _projection(self, stage):
        w = self.w
        self.ctx.enqueue_search_by_projection_kf_batch(0, w["fr"]["bounds"], self.d_cands[stage].data_ptr(), self.K, w["max_kf_n"], 1, 1, self.new[stage].ptr,
                                                       self.nadd[stage].ptr, self.proj_status[stage].ptr, self.has.ptr, self.Xw.ptr, self.st.cuda_stream)
        self._snap("proj%d" % stage)

    def run(self):
        import torch
        ctx, st, w, K, cap, o = self.ctx, self.st, self.w, self.K, self.cap, self.pnp
        s = st.cuda_stream
        ctx.enqueue_stereo(self.d_img.data_ptr(), 1, s)                                            # 1
        self.fv.enqueue(ctx, 0, WS.BOW_LEVEL, st, per_feature=False)                              # 2
        ctx.enqueue_search_by_bow_batch(0, self.d_bow.data_ptr(), K, w["max_kf_nnodes"], self.fv.nodes.ptr, self.fv.node_off.ptr, self.fv.node_feat.ptr,
                                        self.fv.n_nodes.ptr, WS.BOW_RATIO, WS.BOW_ORI, self.f_match.ptr, self.nm.ptr, self.bow_status.ptr,
                                        d_has_point=self.has.ptr, d_Xw=self.Xw.ptr, stream=s)            # 3
        self._snap("bow")
        p = WS.PNP
        ctx.enqueue_pnp_ransac_batch(0, self.d_pnp.data_ptr(), K, w["max_kf_n"], p["min_inliers"], p["max_its"], p["n_iterations"], p["epsilon"], p["th2"], self.table,
                                     o["n_corr"].ptr, o["n_its"].ptr, o["corr"].ptr, 0, o["hyp"].ptr, o["bits"].ptr, o["refined"].ptr, o["refined_bits"].ptr,
                                     o["events"].ptr, o["n_events"].ptr, o["exhausted"].ptr, o["status"].ptr, stream=s)          # 4
        d_keys = ctx.device_keys_un(0, s)
        with torch.cuda.stream(st):                                 # d_keys_un_rows / d_u_right_rows: the slot's arrays once per candidate
            self.keys_rows.copy_(raw(d_keys, 28 * cap).repeat(K))
            self.ur_rows.copy_(raw(device_buffers(ctx)["u_right"], 4 * cap).repeat(K))
        st.synchronize()                                            # 5: the one download, the host picks an event per candidate
        n_events, events = o["n_events"].fetch(), o["events"].fetch().reshape(K, -1)
        self.picks = [WS.pick(dict(n_events=int(n_events[i]), events=events[i])) for i in range(K)]
        for i, (which, k) in enumerate(self.picks):                 # 6
            ctx.enqueue_pnp_ransac_select(0, K, i, which, k, p["max_its"], o["n_corr"].ptr, o["n_its"].ptr, o["corr"].ptr, o["hyp"].ptr, o["bits"].ptr, o["refined"].ptr,
                                          o["refined_bits"].ptr, o["exhausted"].ptr, self.T.ptr + 64 * i, self.cur.ptr + 4 * i * cap, self.has.ptr + i * cap,
                                          self.select_status.ptr + 4 * i, stream=s)
        self._snap("select")
        self._pose(0)                                               # 7
        self._projection(0)                                         # 8
        self._pose(1)                                               # 9
        self._projection(1)                                         # 10
        self._pose(2)                                               # 11
        st.synchronize()
        return self.fetch()

    def fetch(self):
        K, cap = self.K, self.cap
        shape = dict(T=(K, 4, 4), cur=(K, cap), has=(K, cap), Xw=(K, cap, 3), outlier=(K, cap), f_match=(K, cap))
        out = dict(snaps={n: {k: t.cpu().numpy().reshape(shape[k]) for k, t in s.items()} for n, s in self.snaps.items()})
        out["final"] = {k: getattr(self, k).fetch().reshape(shape[k]) for k in STAGE_ROWS + ("f_match",)}      # the guards are checked here
        out.update(nm=self.nm.fetch(), bow_status=self.bow_status.fetch(), select_status=self.select_status.fetch(), picks=list(self.picks),
                   new=[g.fetch().reshape(K, cap) for g in self.new], nadd=[g.fetch() for g in self.nadd], proj_status=[g.fetch() for g in self.proj_status],
                   ngood=[g.fetch() for g in self.ngood])
        f = {k: g.fetch() for k, g in self.pnp.items()}
        mi = WS.PNP["max_its"]
        out["pnp"] = []
        for i in range(K):
            r = {k: int(f[k][i]) for k in ("status", "n_corr", "n_its", "n_events", "exhausted")}
            r.update(corr=f["corr"][i * cap:(i + 1) * cap], **{k: f[k][i * mi:(i + 1) * mi] for k in ("hyp", "bits", "refined", "refined_bits", "events")})
            out["pnp"].append(r)
        return out


def _check_frame(ctx, w, chain):
    """Slot 0 is the world's frame (the extraction equals the oracle bit for bit) and its feature vector the oracle's."""
    fr = w["fr"]
    got = ctx.fetch_image(0, stereo=True)
    assert np.array_equal(got["kps"], fr["k_raw"]) and np.array_equal(got["desc"], fr["d"]) and np.array_equal(got["u_right"], fr["ur"])
    assert np.array_equal(ctx.fetch_keys_un(0), fr["k"])
    chain.fv.check(w["per"], w["fbow"], w["f_fv"], "the frame's feature vector", per_feature=False)


def _verify(w, ids, got, what):
    """Every stage of every candidate against its model on the snapshot from before the stage.  Returns the largest pose difference
    per pose stage."""
    from tests import test_pnp_ransac_device as TP
    from tests.test_pose import POSE_ATOL
    nk = len(w["fr"]["k"])
    S, fin = got["snaps"], got["final"]
    cap = fin["cur"].shape[1]
    worst = [0.0, 0.0, 0.0]
    order = ["bow", "select", "pose0", "proj0", "pose1", "proj1", "pose2"]
    for i, c in enumerate(ids):
        kf, tag = w["cands"][c], "%s, candidate %d" % (what, c)
        # ---- the BoW batch
        m, nm, status, has = WS.stage_bow(w, c)
        b = S["bow"]
        assert int(got["bow_status"][i]) == status and int(got["nm"][i]) == nm, (tag, int(got["bow_status"][i]), int(got["nm"][i]), nm)
        assert np.array_equal(b["f_match"][i, :nk], m), (tag, int((b["f_match"][i, :nk] != m).sum()))
        assert (b["f_match"][i, nk:] == BEYOND).all(), tag                                    # left untouched: the poison is still there
        assert np.array_equal(b["has"][i, :nk], has) and not b["has"][i, nk:].any(), tag
        held = m >= 0
        assert np.array_equal(b["Xw"][i, :nk][held], kf["pos"][m[held]]) and np.isnan(b["Xw"][i, :nk][~held]).all() and np.isnan(b["Xw"][i, nk:]).all(), tag
        assert np.array_equal(fin["f_match"][i], b["f_match"][i]), tag                          # no later stage writes the row
        # ---- PnP on the row where it lies: the model is fed the device's row
        rows = TP._crop(got["pnp"][i], nk)
        TP._assert_same(rows, WS.stage_pnp(w, c, b["f_match"][i, :nk]), tag)
        # ---- select
        which, k = got["picks"][i]
        assert (which, k) == WS.pick(rows)
        T0, cur0, has0, st0 = WS.stage_select(w, rows, which, k, cap, BEYOND, 0)
        s = S["select"]
        assert int(got["select_status"][i]) == st0, (tag, int(got["select_status"][i]), st0)
        assert _same_bits(s["T"][i].reshape(16), T0) and np.array_equal(s["cur"][i], cur0) and np.array_equal(s["has"][i], has0), tag
        assert _same_bits(s["Xw"][i], b["Xw"][i]) and np.array_equal(s["outlier"][i], b["outlier"][i]), tag    # the BoW batch's d_Xw row stays as it is
        # ---- the refinement
        for n, name in enumerate(order[2:], 2):
            before, after = S[order[n - 1]], S[name]
            stage = int(name[-1])
            if name.startswith("pose"):
                T, outl, n_in, trace = WS.stage_pose(w, before["T"][i], before["has"][i], before["Xw"][i], before["outlier"][i])
                d = float(np.abs(after["T"][i] - T).max())
                worst[stage] = max(worst[stage], d)
                assert int(got["ngood"][stage][i]) == n_in, (tag, name, int(got["ngood"][stage][i]), n_in)
                assert np.array_equal(after["outlier"][i, :nk], outl), (tag, name, np.nonzero(after["outlier"][i, :nk] != outl)[0][:8])
                assert (after["outlier"][i, nk:] == 1).all(), (tag, name)
                assert d <= POSE_ATOL, (tag, name, d)
                if n_in == 0:
                    assert _same_bits(after["T"][i], before["T"][i]), (tag, name)              # fewer than 3 correspondences: the pose is left as it is
                for key in ("cur", "has", "Xw"):
                    assert _same_bits(after[key][i], before[key][i]), (tag, name, key)
            else:
                e = WS.stage_projection(w, c, before["T"][i], before["cur"][i], before["outlier"][i] if stage == 0 else None, stage)
                new = got["new"][stage][i]
                assert int(got["proj_status"][stage][i]) == e["status"] == 0 and int(got["nadd"][stage][i]) == e["nm"], (tag, name, int(got["nadd"][stage][i]), e["nm"])
                assert np.array_equal(new[:nk], e["match"]) and (new[nk:] == UNTOUCHED).all(), (tag, name, np.nonzero(new[:nk] != e["match"])[0][:8])
                assert np.array_equal(after["cur"][i, :nk], e["cur_point"]) and (after["cur"][i, nk:] == BEYOND).all(), (tag, name)
                assert np.array_equal(after["has"][i, :nk], e["has"]) and not after["has"][i, nk:].any(), (tag, name)
                h = e["has"] != 0
                assert np.array_equal(after["Xw"][i, :nk][h], kf["pos"][e["cur_point"][h]]), (tag, name)
                assert _same_bits(after["Xw"][i, :nk][~h], before["Xw"][i, :nk][~h]) and np.isnan(after["Xw"][i, nk:]).all(), (tag, name)   # rows without a point untouched
                assert _same_bits(after["T"][i], before["T"][i]) and np.array_equal(after["outlier"][i], before["outlier"][i]), (tag, name)
        for key in STAGE_ROWS:
            assert _same_bits(fin[key][i], S["pose2"][key][i]), (tag, key)
    print("%s: largest |pose - oracle| per pose stage %s; inliers %s; new matches %s" % (
        what, ["%.2e" % v for v in worst], [g.tolist() for g in got["ngood"]], [g.tolist() for g in got["nadd"]]))
    return worst


def _equal_runs(a, b, rows_a, rows_b, poses):
    """Rows rows_a of run a equal rows rows_b of run b bit for bit; poses: the d_Tcw rows too."""
    ia, ib = list(rows_a), list(rows_b)
    for name in a["snaps"]:
        for key in a["snaps"][name]:
            if key != "T" or poses:
                assert _same_bits(a["snaps"][name][key][ia], b["snaps"][name][key][ib]), (name, key)
    for key in ("nm", "bow_status", "select_status"):
        assert np.array_equal(a[key][ia], b[key][ib]), key
    for key in ("new", "nadd", "proj_status", "ngood"):
        for x, y in zip(a[key], b[key]):
            assert np.array_equal(x[ia], y[ib]), key
    for i, j in zip(ia, ib):
        assert a["picks"][i] == b["picks"][j]
        for key, x in a["pnp"][i].items():
            y = b["pnp"][j][key]
            assert _same_bits(x, y) if isinstance(x, np.ndarray) else x == y, ("pnp", key)


def _context(api, distorted):
    ctx = context(api, nfeatures=1500)
    if distorted:
        ctx.set_distortion(WS.DIST)
    B.vocab_load(ctx, WS.vocab())
    return ctx


@pytest.mark.gpu
@pytest.mark.parametrize("distorted", [False, True], ids=["plain", "distortion_set"])
def test_gpu_chain_in_a_fresh_context_and_again(distorted):
    """(a) The context is made for this test and has made no call but the vocabulary's upload (and set_distortion): the BoW, match,
    PnP and pose states are created, and their scratches grow, in the middle of the queued stream.  (b) The same chain again in the same
    context with fresh arrays.  Both are verified stage by stage; (b) equals (a) bit for bit in everything but the poses, for which the
    POSE_ATOL rule holds in each run.  With distortion set, PnP, the pose rows and the projection read the undistorted keys."""
    import torch
    from orbslam2_amd import api
    w = WS.reloc_world(distorted)
    ctx = _context(api, distorted)
    st = torch.cuda.Stream()
    assert ctx.capacity > len(w["fr"]["k"]) and np.array_equal(ctx.tables()["sigma2"][:WS.NL], w["fr"]["sigma2"])
    first = _Chain(api, ctx, st, w, range(4))
    a = first.run()
    _check_frame(ctx, w, first)
    _verify(w, range(4), a, "fresh context")
    second = _Chain(api, ctx, st, w, range(4))
    b = second.run()
    _verify(w, range(4), b, "second run")
    _equal_runs(a, b, range(4), range(4), poses=False)
    ctx.close()


@pytest.mark.gpu
def test_gpu_rows_are_isolated_and_dead_candidates_run_every_stage():
    """Candidates 0 and 1 are bit-identical (poses included) to a run of the same chain with only those two.  Candidates 2 and 3 get
    ORBFE_ERR_INVALID from select, keep the identity and 0 inliers through the first pose call, and their later rows equal what the
    SYNCHRONOUS entry points give for the same inputs: search_by_projection_kf on the resident frame, pose_optimization on the host's
    copies (flags and counts equal, pose within POSE_ATOL)."""
    import torch
    from orbslam2_amd import api
    from tests import test_reloc_projection_device as TR
    from tests.test_pose import POSE_ATOL
    w = WS.reloc_world(False)
    fr, nk = w["fr"], len(w["fr"]["k"])
    ctx = _context(api, False)
    st = torch.cuda.Stream()
    four = _Chain(api, ctx, st, w, range(4)).run()
    two = _Chain(api, ctx, st, w, range(2)).run()
    _verify(w, range(2), two, "candidates 0 and 1 alone")
    _equal_runs(four, two, (0, 1), (0, 1), poses=True)
    S = four["snaps"]
    eye = np.eye(4, dtype=np.float32)
    assert four["bow_status"].tolist() == [0, 0, 0, WS.ERR_INVALID] and four["select_status"].tolist() == [0, 0, WS.ERR_INVALID, WS.ERR_INVALID]
    for c in (2, 3):
        kf = w["cands"][c]
        assert four["pnp"][c]["n_its"] == 0 and four["pnp"][c]["n_events"] == 0
        assert _same_bits(S["select"]["T"][c], eye) and _same_bits(S["pose0"]["T"][c], eye) and int(four["ngood"][0][c]) == 0
        assert (S["select"]["cur"][c, :nk] == -1).all() and not S["select"]["has"][c].any() and not S["pose0"]["outlier"][c, :nk].any()
        for stage, (th, od) in enumerate(WS.STAGES):
            before = S["pose%d" % stage]
            rec = dict(T=before["T"][c], pos=kf["pos"], desc=kf["d"], valid=kf["valid"], angle=kf["ang"], max_d=kf["max_d"], min_d=kf["min_d"], th=th, od=od)
            m, n = TR._sync_kf(ctx, fr, rec, before["cur"][c, :nk], before["outlier"][c, :nk] if stage == 0 else None, 1, True)
            assert n == int(four["nadd"][stage][c]) and np.array_equal(m, four["new"][stage][c][:nk]), (c, stage)
            after = S["proj%d" % stage]
            X = np.where(after["has"][c, :nk, None] != 0, after["Xw"][c, :nk], np.float32(0))
            T, outl, n_in = ctx.pose_optimization(after["T"][c], fr["k"], fr["ur"], after["has"][c, :nk], X, outlier=after["outlier"][c, :nk])
            got = S["pose%d" % (stage + 1)]
            assert n_in == int(four["ngood"][stage + 1][c]) and np.array_equal(outl, got["outlier"][c, :nk]), (c, stage)
            assert np.abs(T - got["T"][c]).max() <= POSE_ATOL, (c, stage)
        assert int(four["nadd"][0][c]) > 0                              # the projection row of the identity pose is a real search
    ctx.close()
