"""LoopClosing::ComputeSim3 end to end on one stream, as INTEGRATION.md tells an integrator to queue it: search_by_bow_kf_batch ->
sim3_ransac_batch (its records hold pairs = d_pairs + i * 2 * n1 and n_pairs = d_nmatches + i, the count still on the device, max_pairs
= n1) -> one download of the events -> for the first event of every candidate that has one: select -> search_by_sim3 ->
optimize_sim3 -> a torch op on the stream that turns match12 into d_kf_matched (and the points' validity) -> the fetch of S12 -> Scw
composed on the host as src/LoopClosing.cc:385-411 does -> search_by_projection_sim3.  The world is tests/world_scenes.py::loop_world
(checked on the CPU by tests/test_world_scenes.py): candidates 0 and 1 are live, candidate 2 has fewer than 20 pairs (n_its = 0).

As in tests/test_chain_relocalization.py the seams are what is pinned: d_pairs holds poison (device_arrays.BEYOND) from 2 * count on,
which must reach no result and still be there afterwards; every stage is verified on its own, its existing model
(tests/world_scenes.py::loop_*) fed the DEVICE's rows from before that stage; everything is compared exactly and nothing is left out
but S12, which is compared within SIM3_ATOL of tests/test_sim3_opt_device.py.  The chain runs in a context that has made no other call
and again in the same context.

Largest |S12 - model| as printed on the MI355X: 2.9e-08 for candidate 0, 1.4e-08 for candidate 1, in both runs.
"""
import numpy as np
import pytest

from orbslam2_amd import bow as B
from tests import sim3_solver_model as SM
from tests import world_scenes as WS
from tests.device_arrays import BEYOND, UNTOUCHED, Guarded, context, upload, upload_records

PAD = 64


class _Chain:
    """KF1, the candidates and every output of one ComputeSim3 in HBM: inputs between PAD readable entries, outputs between guard rows."""

    def __init__(self, api, ctx, st, w):
        import torch
        from tests import test_bow_kf_device as TBK
        from tests import test_fuse_device as TF
        from tests import test_sim3_device as TS
        from tests import test_sim3_ransac_device as TSR
        self.api, self.ctx, self.st, self.w = api, ctx, st, w
        s, n1, n2, K = w["s"], w["n1"], w["n2"], len(w["cands"])
        self.K, self.mi = K, WS.SIM3["max_its"]
        self.own = []
        up = self._up
        # step 1 of INTEGRATION.md: what the keyframes own since they were made (arrays, grids, records)
        self.bow1 = TBK._Kf(api, w["kf1"])
        self.grid1 = TF._Kf(api, ctx, st, s["k1"], s["d1"], None, s["bounds"], s["keyframe"])
        self.pts1 = TS._pts_dev(s["pts1"])
        self.d_pos1, self.d_valid1 = up(w["pos1"]), up(w["valid1"])
        self.table_its = up(w["its_for_n"])
        self.bow2, self.grid2, self.pts2, self.tables, self.d_pos2, self.d_valid2 = [], [], [], [], [], []
        recs = []
        self.match12 = Guarded.cells(K * n1)
        self.pairs = Guarded.cells(K * 2 * n1, BEYOND)              # entries from 2 * count on are never written: the poison stays
        self.nm, self.bow_status = Guarded.cells(K), Guarded.cells(K)
        for i, c in enumerate(w["cands"]):
            self.bow2.append(TBK._Kf(api, c["bow"]))
            g = TF._Kf(api, ctx, st, c["k"], c["d"], None, s["bounds"], s["keyframe"])
            self.grid2.append(g)
            self.pts2.append(TS._pts_dev((c["pos"], c["max_d"], c["min_d"], c["d"], c["valid"])))
            self.tables.append(TF._Table(dict(pos=c["pos"], normal=c["normal"], max_d=c["max_d"], min_d=c["min_d"], desc=c["d"])))
            self.d_pos2.append(up(c["pos"])); self.d_valid2.append(up(c["valid"]))
            r = api.Sim3RansacCandidate()
            r.keys_un, r.pos, r.valid, r.T2w = g.keys.data_ptr(), self.d_pos2[i], self.d_valid2[i], up(c["T2w"].reshape(-1))
            r.pairs, r.n_pairs = self.pairs.ptr + 4 * i * 2 * n1, self.nm.ptr + 4 * i   # row i and its count where the BoW batch leaves them
            r.draws, r.n = up(np.ascontiguousarray(c["draws"], np.uint32).view(np.int32)), n2
            recs.append(r)
        self.d_bow = TBK._rec_array(self.bow2)
        self.d_cands = upload_records(recs)
        f, mi, words = TSR._filled, self.mi, (n1 + 31) // 32
        self.ransac = dict(n_corr=Guarded(f(K, np.int32)), n_its=Guarded(f(K, np.int32)), corr=Guarded(f((K * n1, 2), np.int32)), hyp=Guarded(f(K * mi, SM.HYP_DTYPE)),
                           bits=Guarded(f((K * mi, words), np.uint32)), events=Guarded(f(K * mi, np.int32)), n_events=Guarded(f(K, np.int32)),
                           status=Guarded(f(K, np.int32)))
        self.sel = [TSR._Select(n1, w["max_kf_n"]) for _ in range(K)]
        self.out12 = [TS._Out12(n1) for _ in range(K)]
        self.S12 = [Guarded(np.full(8, np.nan)) for _ in range(K)]
        self.n_in, self.opt_status = [Guarded.cells(1) for _ in range(K)], [Guarded.cells(1) for _ in range(K)]
        self.kf_matched = [torch.full((n1 + PAD,), 7, dtype=torch.uint8, device="cuda:0") for _ in range(K)]
        self.pt_valid = [torch.full((n2 + PAD,), 7, dtype=torch.int32, device="cuda:0") for _ in range(K)]
        self.proj = [TS._OutProj(n2, n1) for _ in range(K)]
        self.t_valid2 = [upload(np.ascontiguousarray(c["valid"], np.int32))[0] for c in w["cands"]]
        self.by_sim3 = {}
        torch.cuda.synchronize()

    def _up(self, a):
        t, p = upload(a, front=PAD, pad=PAD)
        self.own.append(t)
        return p

    def run(self):
        import torch
        ctx, st, w, K, o = self.ctx, self.st, self.w, self.K, self.ransac
        n1, n2, s = w["n1"], w["n2"], st.cuda_stream
        ctx.enqueue_search_by_bow_kf_batch(self.bow1.rec, self.d_bow.data_ptr(), K, w["max_kf_n"], WS.BOW_RATIO, WS.BOW_ORI, self.match12.ptr, self.nm.ptr,
                                           self.bow_status.ptr, d_pairs=self.pairs.ptr, stream=s)                                       # 1
        ctx.enqueue_sim3_ransac_batch(self.grid1.rec, w["T1w"], self.d_pos1, self.d_valid1, self.d_cands.data_ptr(), K, n1, w["max_kf_n"], WS.SIM3["fix_scale"],
                                      WS.SIM3["min_inliers"], self.mi, self.table_its, o["n_corr"].ptr, o["n_its"].ptr, o["corr"].ptr, 0, o["hyp"].ptr, o["bits"].ptr,
                                      o["events"].ptr, o["n_events"].ptr, o["status"].ptr, stream=s)                                      # 2
        st.synchronize()                                                                                                                  # 3
        n_events, events, hyp = o["n_events"].fetch(), o["events"].fetch().reshape(K, -1), o["hyp"].fetch().reshape(K, -1)
        self.live = [(i, int(events[i, 0])) for i in range(K) if n_events[i] > 0]
        for i, k in self.live:                                                                                                            # 4
            h, c, sel, out = hyp[i, k], w["cands"][i], self.sel[i], self.out12[i]
            ctx.enqueue_sim3_ransac_select(self.d_cands.data_ptr(), K, i, k, n1, self.d_valid1, n1, w["max_kf_n"], self.mi, o["n_corr"].ptr, o["n_its"].ptr, o["corr"].ptr,
                                           o["bits"].ptr, sel.prior.ptr, sel.v1.ptr, sel.v2.ptr, sel.status.ptr, stream=s)
            ctx.enqueue_search_by_sim3(self.grid1.rec, w["T1w"], [t.data_ptr() for t in self.pts1[:4]] + [sel.v1.ptr], self.grid2[i].rec, c["T2w"],
                                       [t.data_ptr() for t in self.pts2[i][:4]] + [sel.v2.ptr], h["s12"], h["R12"], h["t12"], WS.SIM3_TH, *out.ptrs(), stream=s)
            with torch.cuda.stream(st):
                self.by_sim3[i] = out.match.view.clone()            # OptimizeSim3 rewrites d_match12 in place
            ctx.enqueue_optimize_sim3(self.grid1.rec, w["T1w"], self.d_pos1, self.d_valid1, self.grid2[i].rec, c["T2w"], self.d_pos2[i], self.d_valid2[i], h["s12"], h["R12"],
                                      h["t12"], WS.OPT_TH2, WS.SIM3["fix_scale"], out.match.ptr, self.S12[i].ptr, self.n_in[i].ptr, self.opt_status[i].ptr,
                                      d_prior12=sel.prior.ptr, stream=s)
            with torch.cuda.stream(st):                                                                                                   # 5
                m = out.match.view
                self.kf_matched[i][:n1] = (m >= 0).to(torch.uint8)
                found = torch.zeros(n2 + 1, dtype=torch.int32, device="cuda:0")
                found.scatter_(0, torch.where(m >= 0, m, torch.full_like(m, n2)).long(), torch.ones_like(m))
                self.pt_valid[i][:n2] = ((self.t_valid2[i] != 0) & (found[:n2] == 0)).to(torch.int32)
        st.synchronize()                                            # the fetch of S12
        self.Scw = {}
        for i, k in self.live:                                                                                                            # 6
            self.Scw[i] = WS.loop_scw(w, i, self.S12[i].fetch())
            ctx.enqueue_search_by_projection_sim3(self.grid1.rec, self.Scw[i], n2, 0, n2, *self.tables[i].ptrs(), self.pt_valid[i].data_ptr(), self.kf_matched[i].data_ptr(),
                                                  WS.LOOP_TH, *self.proj[i].ptrs(), stream=s)
        st.synchronize()
        return self.fetch()

    def fetch(self):
        K, n1, mi = self.K, self.w["n1"], self.mi
        got = dict(match12=self.match12.fetch().reshape(K, n1), pairs=self.pairs.fetch().reshape(K, 2 * n1), nm=self.nm.fetch(), bow_status=self.bow_status.fetch(),
                   live=list(self.live))
        f = {k: g.fetch() for k, g in self.ransac.items()}
        got["ransac"] = [dict(status=int(f["status"][i]), n_corr=int(f["n_corr"][i]), n_its=int(f["n_its"][i]), n_events=int(f["n_events"][i]),
                              corr=f["corr"][i * n1:(i + 1) * n1], hyp=f["hyp"][i * mi:(i + 1) * mi], bits=f["bits"][i * mi:(i + 1) * mi],
                              events=f["events"][i * mi:(i + 1) * mi]) for i in range(K)]
        got["round"] = {}
        for i, k in self.live:
            n2 = self.w["n2"]
            got["round"][i] = dict(k=k, select=self.sel[i].fetch(), by_sim3=(self.by_sim3[i].cpu().numpy(), int(self.out12[i].count.fetch()[0]), int(self.out12[i].status.fetch()[0])),
                                   match12=self.out12[i].match.fetch(), S12=self.S12[i].fetch(), n_inliers=int(self.n_in[i].fetch()[0]), opt_status=int(self.opt_status[i].fetch()[0]),
                                   kf_matched=self.kf_matched[i].cpu().numpy(), pt_valid=self.pt_valid[i].cpu().numpy(), proj=self.proj[i].fetch(), Scw=self.Scw[i])
        dead = [i for i in range(K) if i not in dict(self.live)]
        got["dead_untouched"] = all(g.untouched() for i in dead for g in (self.sel[i].prior, self.sel[i].v1, self.sel[i].v2, self.out12[i].match, self.S12[i], self.proj[i].pt))
        for g in self.grid2 + [self.grid1]:
            g.off.fetch(), g.idx.fetch()                            # the grids' guards
        return got


def _verify(w, got, what):
    from tests import test_sim3_ransac_device as TSR
    from tests.test_sim3_opt_device import POSE_ATOL, SIM3_ATOL, _s12_diff
    n1, n2 = w["n1"], w["n2"]
    worst = 0.0
    for i in range(len(w["cands"])):
        tag = "%s, candidate %d" % (what, i)
        # ---- the BoW batch
        m, pairs, nm = WS.loop_bow(w, i)
        assert int(got["bow_status"][i]) == 0 and int(got["nm"][i]) == nm and np.array_equal(got["match12"][i], m), tag
        assert np.array_equal(got["pairs"][i, :2 * nm], pairs[:2 * nm]) and (got["pairs"][i, 2 * nm:] == BEYOND).all(), tag    # the poison is still there
        # ---- RANSAC on the row and the count where they lie: the model is fed the device's pairs
        rows = got["ransac"][i]
        TSR._assert_same(rows, WS.loop_ransac(w, i, got["pairs"][i, :2 * nm]), tag)
        if i not in got["round"]:
            assert rows["n_events"] == 0, tag
            continue
        r = got["round"][i]
        k, hyp = r["k"], rows["hyp"][r["k"]]
        assert k == int(rows["events"][0])
        # ---- select
        prior, v1, v2, status = r["select"]
        rp, r1, r2 = WS.loop_select(w, i, rows, k)
        assert status == 0 and np.array_equal(prior, rp) and np.array_equal(v1, r1) and np.array_equal(v2[:n2], r2) and (v2[n2:] == UNTOUCHED).all(), tag
        # ---- SearchBySim3 on the round's arrays
        ref, nref = WS.loop_by_sim3(w, i, hyp, v1, v2)
        assert r["by_sim3"][2] == 0 and r["by_sim3"][1] == nref and np.array_equal(r["by_sim3"][0], ref), (tag, r["by_sim3"][1], nref)
        # ---- OptimizeSim3 on what the two calls before it left
        opt = WS.loop_optimize(w, i, hyp, prior, r["by_sim3"][0])
        d = _s12_diff(r["S12"], opt["S12"])
        worst = max(worst, d)
        assert r["opt_status"] == opt["status"] == 0 and r["n_inliers"] == opt["n_inliers"] and np.array_equal(r["match12"], opt["match12"]), (tag, r["n_inliers"], opt["n_inliers"])
        assert d <= SIM3_ATOL <= POSE_ATOL, (tag, d)
        # ---- the projection on the optimiser's surviving matches and the fetched S12
        kf_matched, pt_valid = WS.loop_projection_inputs(w, i, r["match12"])
        assert np.array_equal(r["kf_matched"][:n1], kf_matched) and (r["kf_matched"][n1:] == 7).all(), tag
        assert np.array_equal(r["pt_valid"][:n2], pt_valid) and (r["pt_valid"][n2:] == 7).all(), tag
        pref, npref = WS.loop_projection(w, i, r["Scw"], kf_matched, pt_valid)
        pt, kf, count, pstatus = r["proj"]
        inverse = np.full(n1, -1, np.int32)
        inverse[pref[pref >= 0]] = np.nonzero(pref >= 0)[0]
        assert pstatus == 0 and count == npref and np.array_equal(pt, pref) and np.array_equal(kf, inverse), (tag, count, npref)
        print("%s: hypothesis %d, %d RANSAC inliers, SearchBySim3 %d, OptimizeSim3 keeps %d, |S12 - model| %.2e, the projection adds %d" % (
            tag, k, hyp["n_inliers"], nref, r["n_inliers"], d, count))
    assert got["dead_untouched"]
    return worst


def _flat(got):
    """Every array of a run except S12 (and Scw, which is formed from it), for the bit comparison of two runs."""
    out = [got["match12"], got["pairs"], got["nm"], got["bow_status"], np.array(got["live"])]
    for r in got["ransac"]:
        out += [np.asarray(v) for _, v in sorted(r.items())]
    for i in sorted(got["round"]):
        r = got["round"][i]
        out += list(r["select"][:3]) + [np.array([r["select"][3], r["by_sim3"][1], r["by_sim3"][2], r["n_inliers"], r["opt_status"], r["proj"][2], r["proj"][3]])]
        out += [r["by_sim3"][0], r["match12"], r["kf_matched"], r["pt_valid"], r["proj"][0], r["proj"][1]]
    return out


@pytest.mark.gpu
def test_gpu_chain_in_a_fresh_context_and_again():
    """(a) In a context that has made no call but the vocabulary's upload and the keyframes' grids, so that the BoW, RANSAC, matcher and
    optimiser states are created mid-chain; (b) again in the same context.  Both verified stage by stage; (b) equals (a) bit for bit in
    everything but S12.  Candidate 2 reports n_its == 0, gets no round, and none of its rows is written."""
    import torch
    from orbslam2_amd import api
    w = WS.loop_world()
    ctx = context(api)
    B.vocab_load(ctx, WS.vocab())
    st = torch.cuda.Stream()
    assert np.array_equal(ctx.tables()["sigma2"][:WS.NL], w["sigma2"])
    a = _Chain(api, ctx, st, w).run()
    assert [i for i, _ in a["live"]] == [0, 1] and a["ransac"][2]["n_its"] == 0 and a["ransac"][2]["n_events"] == 0 and a["ransac"][2]["status"] == 0
    _verify(w, a, "fresh context")
    b = _Chain(api, ctx, st, w).run()
    _verify(w, b, "second run")
    fa, fb = _flat(a), _flat(b)
    assert len(fa) == len(fb) and all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(fa, fb))
    ctx.close()
