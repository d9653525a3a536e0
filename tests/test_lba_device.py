"""orbfe_enqueue_local_bundle_adjustment / orbfe_local_bundle_adjustment (Optimizer::LocalBundleAdjustment, reference
src/Optimizer.cc:566-822; orbslam2_amd/csrc/orbfe_lba.hip) against the float64 model (tests/lba_model.py) on the scenes of
tests/lba_scenes.py, which tests/test_lba_model.py has checked on the CPU: every scene keeps 1 % distance from 5.991 / 7.815 and a depth
margin at both classifications, so d_edge_code, d_erase, the counts, d_info.iterations and d_status are compared EXACTLY and no edge is
left out of any comparison.

Scenes: mixed (4 local, one of them held, 2 fixed, 64-slot keyframes, 40 points, 160 edges, a tenth gross outliers), mono, stereo, behind
(edges flagged by depth alone), orphans (points and a local keyframe without a level-0 edge in round 2), stale (round 2 ends on rejected
trials), skip (a role-0 keyframe), rows (d_row given, the other rows checked), reduced_hbm (ORBFE_LBA_LDS_KEYFRAMES + 1 free keyframes in
a chain: the reduced system in HBM), faulty_* (one per device-visible fault, a descending offset among them: equal to the model without
those edges), empty and all_skipped (no edge at all), and the boundary scenes of the kernel's strides (LBA_THREADS = 512 threads, 8
waves, index batches of 64): points_511/512/513, edges_511/512/513, free_7/8/9, free_20/21 (+ reduced_hbm = 22), views_63/64/65 (one
point observed by that many keyframes, a free one last in its list: the Schur rows fetch a point's list 64 entries at a time) and
kf_edges_63/64/65 (a free keyframe with that many edges, all at level 0: both keyframe walks fetch its edges 64 at a time).

Tolerances: each bound is 8 x the largest |device - model| over all scenes of this file on the MI355X, rounded up to one digit.
    quantity                                             largest difference                                  bound
    pose (entries of R, t in metres of the float rows)   1.863e-09  (points_511; 0 in 34 of the 35 scenes)   POSE_ATOL  = 2e-8
    point position (metres, float rows)                  5.960e-08  (points_513; 0 in 33 of the 35 scenes)   POINT_ATOL = 5e-7
    d_edge_chi2, relative (|d - m| / max(m, 1))          2.489e-06  (points_511; below 4e-8 on 32 scenes)    CHI2_RTOL  = 2e-5
The outputs are floats: almost everywhere the two double estimates round
to the same float, and the two non-zero maxima are one float ulp of one entry.  The chi2 maximum belongs to the 511-point scene, whose
points have two views each and whose second round uses all ten iterations without settling: a weakly determined minimum.  The factor
covers the spread the header of tests/test_pose.py documents (the stop rules compare nearly equal
chi2 values).  Pose and point bounds may not exceed that file's 1e-5; a larger difference would mean a flipped decision, to be found
through the iteration and trial counts this file prints, not accepted.  chi2 is relative on the scale of the thresholds it is compared
with: below 1 it is measured against 1.

Device arrays and guards follow tests/device_arrays.py: inputs between PAD readable entries, every output between sentinel rows and
started from a sentinel value, never the default stream.
"""
import ctypes as C

import numpy as np
import pytest

from tests import lba_model as M
from tests import lba_scenes as S
from tests import map_point_model as MP
from tests.device_arrays import UNTOUCHED, Guarded, context, upload

PAD = 64
POSE_ATOL = 2e-8    # see the header: 8 x the measured maxima, rounded up to one digit
POINT_ATOL = 5e-7
CHI2_RTOL = 2e-5
CEILING = 1e-5      # tests/test_pose.py


@pytest.fixture(scope="module")
def gpu():
    import torch
    from orbslam2_amd import api
    ctx = context(api)
    assert np.array_equal(ctx.tables()["inv_sigma2"][:S.NLEVELS], S.INV_SIGMA2)
    assert api.LBA_LDS_KEYFRAMES == S.LDS_KEYFRAMES
    yield api, ctx, torch.cuda.Stream()
    ctx.close()


class _Call:
    """One scene in HBM: inputs uploaded once, fresh guarded outputs."""

    def __init__(self, api, s, chi2=True, obs_kfs=True):
        import torch
        self.s, self.own = s, []
        n_kfs, n_obs = len(s["role"]), len(s["obs_kf"])

        def up(a):
            t, p = upload(a, front=PAD, pad=PAD)
            self.own.append(t)
            return p
        rec = np.zeros(n_kfs, np.dtype([("keys_un", "<u8"), ("u_right", "<u8"), ("n", "<i4"), ("reserved", "<i4", 3)]))
        for k, (keys, ur) in enumerate(s["kfs"]):
            rec["keys_un"][k], rec["u_right"][k], rec["n"][k] = up(keys), up(ur), len(keys)
        self.rec_np, self.rec = rec, up(rec)
        self.role = up(s["role"])
        self.row = 0 if s["row"] is None else up(s["row"])
        self.off, self.okf, self.oidx = up(s["obs_off"]), up(s["obs_kf"]), up(s["obs_idx"])
        self.Tcw, self.pos = Guarded(s["Tcw"]), Guarded(s["pos"])
        dirs = np.zeros(n_kfs, api.OBS_KF_DTYPE)
        dirs["desc"], dirs["keys_un"], dirs["n"], dirs["bad"], dirs["reserved"] = 0x1111, 0x2222, 77, 5, 9
        dirs["Ow"] = np.arange(3 * n_kfs, dtype=np.float32).reshape(n_kfs, 3) + 1000
        self.dirs0 = dirs
        self.dirs = Guarded(dirs) if obs_kfs else None
        self.code = Guarded(np.full(n_obs, 0xEE, np.uint8), guard_rows=PAD)
        self.chi2 = Guarded(np.full(n_obs, -7.0)) if chi2 else None
        self.erase = Guarded(np.full((n_obs, 2), UNTOUCHED, np.int32))
        self.n_erase, self.status = Guarded.cells(1), Guarded.cells(1)
        self.info = Guarded(np.frombuffer(bytes([0xEE]) * 64, api.LBA_INFO_DTYPE).copy())
        torch.cuda.synchronize()   # the uploads and fills above ran on torch's own stream

    def enqueue(self, ctx, st, max_free=None):
        s = self.s
        ctx.enqueue_local_bundle_adjustment(self.rec, self.role, len(s["role"]), s["max_free"] if max_free is None else max_free, self.Tcw.ptr,
                                            len(s["obs_off"]) - 1, self.row, s["n_rows"], self.off, self.okf, self.oidx, len(s["obs_kf"]),
                                            self.pos.ptr, self.dirs.ptr if self.dirs else 0, self.code.ptr, self.chi2.ptr if self.chi2 else 0,
                                            self.erase.ptr, self.n_erase.ptr, self.info.ptr, self.status.ptr, stream=st.cuda_stream)

    def fetch(self):
        return dict(Tcw=self.Tcw.fetch(), pos=self.pos.fetch(), dirs=self.dirs.fetch() if self.dirs else None, edge_code=self.code.fetch(),
                    edge_chi2=self.chi2.fetch() if self.chi2 else None, erase=self.erase.fetch(), n_erase=int(self.n_erase.fetch()[0]),
                    info=self.info.fetch()[0], status=int(self.status.fetch()[0]))

    def all_outputs_untouched(self):
        return all(g.untouched() for g in (self.Tcw, self.pos, self.dirs, self.code, self.chi2, self.erase, self.n_erase, self.info) if g is not None)


def _alone(gpu, name, **kw):
    api, ctx, st = gpu
    c = _Call(api, S.scene(name), **kw)
    c.enqueue(ctx, st)
    st.synchronize()
    return c.fetch()


def _bits(a):
    return tuple(None if v is None else (v.tobytes() if hasattr(v, "tobytes") else v) for _, v in sorted(a.items()))


def _compare(name, s, got, ref):
    """Exact: status, codes, erase list, counts, iterations, untouched rows, Ow.  Within the measured bounds: poses, points, chi2.
    Returns the three measured differences."""
    n_obs = len(s["obs_kf"])
    info = got["info"]
    ran = ref["info"]["n_mono"] + ref["info"]["n_stereo"] > 0
    print("%-14s status %2d edges %4d+%4d free %2d points %3d  iterations %s (model %s) trials %s (model %s) erased %d" % (
        name, got["status"], info["n_mono"], info["n_stereo"], info["n_free"], info["n_points"], info["iterations"].tolist(), ref["iterations"],
        info["trials"].tolist(), ref["trials"], got["n_erase"]))
    assert got["status"] == ref["status"], name
    assert np.array_equal(got["edge_code"], ref["edge_code"]), (name, np.nonzero(got["edge_code"] != ref["edge_code"])[0][:8])
    for f in ("n_mono", "n_stereo", "n_free", "n_points"):
        assert info[f] == ref["info"][f], (name, f)
    assert info["iterations"].tolist() == ref["iterations"], name
    assert got["n_erase"] == len(ref["erase"]) and np.array_equal(got["erase"][:got["n_erase"]], ref["erase"]), name
    assert (got["erase"][got["n_erase"]:] == UNTOUCHED).all(), name
    rew = ref["rewritten"]
    assert got["Tcw"][~rew].tobytes() == s["Tcw"][~rew].tobytes(), name                     # roles 0 and 3 keep their bits
    named = np.zeros(s["n_rows"], bool)
    if ran:
        ok = np.nonzero(M.build(s["kfs"], s["role"], s["Tcw"], s["row"], s["n_rows"], s["obs_off"], s["obs_kf"], s["obs_idx"], s["pos"], S.INV_SIGMA2,
                                S.NLEVELS).pt_ok)[0]
        named[(np.arange(len(s["obs_off"]) - 1) if s["row"] is None else s["row"])[ok]] = True
    assert got["pos"][~named].tobytes() == s["pos"][~named].tobytes(), name                 # rows no point names keep their bits
    d_pose = float(np.abs(got["Tcw"][rew].astype(np.float64) - ref["Tcw"][rew]).max()) if rew.any() else 0.0
    d_point = float(np.abs(got["pos"][named].astype(np.float64) - ref["pos"][named]).max()) if named.any() else 0.0
    d_chi = 0.0
    if ran:
        d_chi = float((np.abs(got["edge_chi2"] - ref["edge_chi2"]) / np.maximum(ref["edge_chi2"], 1.0)).max())
        for f in ("chi2_start", "chi2_first", "chi2_second"):
            d_chi = max(d_chi, abs(float(info[f]) - ref["info"][f]) / max(ref["info"][f], 1.0))
        assert info["lambda_last"] > 0
    print("    |pose - model| %.3e   |point - model| %.3e   chi2 relative %.3e" % (d_pose, d_point, d_chi))
    assert d_pose <= POSE_ATOL <= CEILING and d_point <= POINT_ATOL <= CEILING and d_chi <= CHI2_RTOL, (name, d_pose, d_point, d_chi)
    if got["dirs"] is not None:                                                              # Ow from the FETCHED rows, bit for bit
        want = got["dirs"].copy()
        for k in np.nonzero(rew)[0]:
            assert got["dirs"]["Ow"][k].tobytes() == M.camera_centre(got["Tcw"][k]).tobytes(), (name, k)
            want["Ow"][k] = 0
        return d_pose, d_point, d_chi, want
    return d_pose, d_point, d_chi, None


@pytest.mark.gpu
@pytest.mark.parametrize("name", S.DEVICE_SCENES)
def test_gpu_scene_against_the_model(gpu, name):
    api = gpu[0]
    s, ref = S.scene(name), S.model(name)
    c = _Call(api, s)
    c.enqueue(gpu[1], gpu[2])
    gpu[2].synchronize()
    got = c.fetch()
    _, _, _, dirs = _compare(name, s, got, ref)
    keep = c.dirs0.copy()
    keep["Ow"][ref["rewritten"]] = 0
    assert dirs.tobytes() == keep.tobytes(), name            # nothing but Ow of the rewritten keyframes is touched in the directory
    if name in S.EMPTY:                                      # no edge at all: status, counts of zero, the codes; nothing else
        assert got["status"] == 0 and got["n_erase"] == 0 and bytes(got["info"].tobytes()) == bytes(64)
        assert c.Tcw.untouched() and c.pos.untouched() and c.dirs.untouched() and c.erase.untouched()
    if name in S.FAULTY:
        assert got["status"] == M.ERR_INVALID
    if name == "behind":                                     # flagged by depth alone: chi2 far below the threshold
        j = np.nonzero(np.isin(s["obs_off"].searchsorted(np.arange(len(s["obs_kf"])), side="right") - 1, [40, 41, 42]))[0]
        assert len(j) == 9 and (got["edge_code"][j] == 3).all() and (got["edge_chi2"][j] < 5.0).all()
    if name == "orphans":
        assert int(got["info"]["n_free"]) == 4 and ref["reduced"] == [24, 18]
    if name == "stale":
        assert ref["last_rejected"] == [False, True]
    if name == "skip":
        assert (got["edge_code"] == 4).sum() > 0 and got["Tcw"][1].tobytes() == s["Tcw"][1].tobytes()
    if name == "mixed":                                      # the held keyframe goes through toSE3Quat -> toCvMat
        assert ref["rewritten"][3] and s["role"][3] == M.LOCAL_HELD


@pytest.mark.gpu
def test_gpu_two_runs_and_back_to_back_calls_give_the_same_bits(gpu):
    """The same inputs give the same bits on every run; two scenes queued back to back on one stream (the second reuses and regrows the
    context's scratch) give what each gives alone."""
    api, ctx, st = gpu
    alone = {n: _alone(gpu, n) for n in ("mixed", "reduced_hbm", "edges_513")}
    for n in alone:
        assert _bits(_alone(gpu, n)) == _bits(alone[n]), n
    for pair in (("mixed", "reduced_hbm"), ("reduced_hbm", "mixed"), ("edges_513", "mixed")):
        calls = [_Call(api, S.scene(n)) for n in pair]
        for c in calls:
            c.enqueue(ctx, st)
        st.synchronize()
        for n, c in zip(pair, calls):
            assert _bits(c.fetch()) == _bits(alone[n]), (pair, n)


@pytest.mark.gpu
def test_gpu_optional_outputs_and_the_capacity_bound(gpu):
    api, ctx, st = gpu
    full = _alone(gpu, "mixed")
    bare = _alone(gpu, "mixed", chi2=False, obs_kfs=False)
    for f in ("Tcw", "pos", "edge_code", "erase", "n_erase", "status"):
        assert np.array_equal(full[f], bare[f]), f
    assert full["info"].tobytes() == bare["info"].tobytes()
    s = S.scene("mixed")
    c = _Call(api, s)
    c.enqueue(ctx, st, max_free=s["max_free"] - 1)           # more role-1 keyframes than the bound: the status and nothing else
    st.synchronize()
    assert int(c.status.fetch()[0]) == api.ERR_CAPACITY and c.all_outputs_untouched()
    c = _Call(api, s)
    c.enqueue(ctx, st, max_free=S.LDS_KEYFRAMES + 1)         # a looser bound picks the HBM variant: the same decisions
    st.synchronize()
    _compare("mixed, system in HBM", s, c.fetch(), S.model("mixed"))


@pytest.mark.gpu
def test_gpu_host_entry_point_equals_the_enqueue_form_bit_for_bit(gpu):
    api, ctx, st = gpu
    for name in ("mixed", "rows", "reduced_hbm", "faulty_obs_idx", "empty"):
        s, dev = S.scene(name), _alone(gpu, name)
        out = ctx.local_bundle_adjustment(s["kfs"], s["role"], s["Tcw"], s["row"], s["n_rows"], s["obs_off"], s["obs_kf"], s["obs_idx"], s["pos"])
        assert out["status"] == dev["status"], name
        assert out["Tcw"].tobytes() == dev["Tcw"].tobytes() and out["pos"].tobytes() == dev["pos"].tobytes(), name
        assert np.array_equal(out["edge_code"], dev["edge_code"]) and out["edge_chi2"].tobytes() == dev["edge_chi2"].tobytes(), name
        assert np.array_equal(out["erase"], dev["erase"][:dev["n_erase"]]) and out["info"].tobytes() == dev["info"].tobytes(), name
        rew = S.model(name)["rewritten"]
        assert out["Ow"][rew].tobytes() == dev["dirs"]["Ow"][rew].tobytes() and np.isnan(out["Ow"][~rew]).all(), name
    # no keyframe, no point, no row, no observation: every padded array of the call is empty; the kernel's "no edge at all" answer
    z = np.zeros(0, np.int32)
    out = ctx.local_bundle_adjustment([], np.zeros(0, np.uint8), np.zeros((0, 16), np.float32), None, 0, np.zeros(1, np.int32), z, z, np.zeros((0, 3), np.float32))
    assert out["status"] == 0 and not any(out["info"].tobytes()) and len(out["erase"]) == 0 and len(out["Tcw"]) == 0 and len(out["edge_code"]) == 0


@pytest.mark.gpu
def test_gpu_host_mirror_equals_the_enqueue_form_bit_for_bit(gpu):
    """ORB_SLAM2::Optimizer::LocalBundleAdjustment of orbslam2_amd/host/Optimizer.h (behind tests/lba_blocks/liblba_wrapper.so): the
    same bits, Ow rows of keyframes that are not rewritten left as the caller had them, an exception on the library's error."""
    import os
    api, ctx, st = gpu
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lba_blocks", "liblba_wrapper.so")
    if not os.path.exists(path):
        raise RuntimeError("tests/lba_blocks/liblba_wrapper.so is missing: __graft_entry__.build() compiles it")
    W = C.CDLL(path)
    vp = C.c_void_p
    W.lba_wrapper_adjust.restype = C.c_int
    W.lba_wrapper_adjust.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp]

    def run(s):
        n_kfs, n_pts, n_obs = len(s["role"]), len(s["obs_off"]) - 1, len(s["obs_kf"])
        keys, ur = np.concatenate([k for k, _ in s["kfs"]]), np.concatenate([u for _, u in s["kfs"]]).astype(np.float32)
        kf_n = np.array([len(k) for k, _ in s["kfs"]], np.int32)
        out = dict(Tcw=s["Tcw"].copy(), Ow=np.full((n_kfs, 3), -7.0, np.float32), pos=s["pos"].copy(), edge_code=np.zeros(n_obs, np.uint8),
                   edge_chi2=np.zeros(n_obs), erase=np.zeros((n_obs + 1, 2), np.int32), info=np.zeros(1, api.LBA_INFO_DTYPE))
        n_erase = C.c_int32()
        p = lambda a: a.ctypes.data_as(vp)
        role = np.ascontiguousarray(s["role"], np.uint8)
        rc = W.lba_wrapper_adjust(ctx.h, n_kfs, p(kf_n), p(keys), p(ur), p(role), p(out["Tcw"]), p(out["Ow"]), n_pts, p(out["pos"]), p(s["obs_off"]),
                                  p(s["obs_kf"]), p(s["obs_idx"]), n_obs, p(out["edge_code"]), p(out["edge_chi2"]), p(out["erase"]), C.byref(n_erase),
                                  p(out["info"]))
        out["erase"] = out["erase"][:n_erase.value]
        return rc, out
    for name in ("mixed", "reduced_hbm"):
        s, dev = S.scene(name), _alone(gpu, name)
        rc, out = run(s)
        assert rc == 0, name
        assert out["Tcw"].tobytes() == dev["Tcw"].tobytes() and out["pos"].tobytes() == dev["pos"].tobytes(), name
        assert np.array_equal(out["edge_code"], dev["edge_code"]) and out["edge_chi2"].tobytes() == dev["edge_chi2"].tobytes(), name
        assert np.array_equal(out["erase"], dev["erase"][:dev["n_erase"]]) and out["info"][0].tobytes() == dev["info"].tobytes(), name
        rew = S.model(name)["rewritten"]
        assert out["Ow"][rew].tobytes() == dev["dirs"]["Ow"][rew].tobytes() and (out["Ow"][~rew] == -7.0).all(), name
    s = S.scene("mixed")
    s["obs_idx"][7] = len(s["kfs"][0][0])                     # the wrapper throws on the library's error
    assert run(s)[0] == -100


@pytest.mark.gpu
def test_gpu_host_visible_errors_queue_nothing(gpu):
    api, ctx, st = gpu
    s = S.scene("mixed")
    c = _Call(api, s)
    good = dict(d_kfs=c.rec, d_role=c.role, n_kfs=len(s["role"]), max_free_kfs=s["max_free"], d_Tcw=c.Tcw.ptr, n_pts=len(s["obs_off"]) - 1, d_row=0,
                n_rows=s["n_rows"], d_obs_off=c.off, d_obs_kf=c.okf, d_obs_idx=c.oidx, n_obs=len(s["obs_kf"]), d_pos=c.pos.ptr, d_obs_kfs=c.dirs.ptr,
                d_edge_code=c.code.ptr, d_edge_chi2=c.chi2.ptr, d_erase=c.erase.ptr, d_n_erase=c.n_erase.ptr, d_info=c.info.ptr, d_status=c.status.ptr)
    for bad in (dict(d_info=0), dict(d_status=0), dict(d_n_erase=0), dict(n_kfs=-1), dict(n_pts=-1), dict(n_obs=-1), dict(n_rows=-1), dict(max_free_kfs=-1),
                dict(n_rows=s["n_rows"] - 1), dict(d_kfs=0), dict(d_role=0), dict(d_Tcw=0), dict(d_obs_off=0), dict(d_pos=0), dict(d_obs_kf=0),
                dict(d_obs_idx=0), dict(d_edge_code=0), dict(d_erase=0)):
        with pytest.raises(api.OrbfeError) as e:
            ctx.enqueue_local_bundle_adjustment(**dict(good, **bad), stream=st.cuda_stream)
        assert e.value.code == api.ERR_INVALID, bad
    st.synchronize()
    assert c.all_outputs_untouched() and c.status.untouched()


@pytest.mark.gpu
def test_gpu_chain_bundle_adjustment_then_update_normal_and_depth(gpu):
    """BA, then orbfe_enqueue_update_map_points(ORBFE_MP_NORMAL_DEPTH) over the same rows with the erased observations removed, on one
    stream with one synchronise for the BA's results: equals tests/map_point_model.py on the fetched positions and Ow exactly."""
    import torch
    api, ctx, st = gpu
    s = S.scene("rows")
    n_kfs, n_pts = len(s["role"]), len(s["obs_off"]) - 1
    c = _Call(api, s)
    dirs = c.dirs0.copy()                                     # a real directory: keys_un of the BA's records, a descriptor buffer nobody reads
    rec = c.rec_np
    desc, desc_ptr = upload(np.zeros((64, 32), np.uint8), PAD, PAD)
    dirs["desc"], dirs["keys_un"], dirs["n"], dirs["bad"] = desc_ptr, rec["keys_un"], rec["n"], 0
    c.dirs, c.dirs0 = Guarded(dirs), dirs
    torch.cuda.synchronize()
    c.enqueue(ctx, st)
    st.synchronize()                                          # the one synchronise: the host erases observations from d_erase
    got = c.fetch()
    erased = set(map(tuple, got["erase"][:got["n_erase"]].tolist()))
    off, okf, oidx = [0], [], []
    for q in range(n_pts):
        for j in range(s["obs_off"][q], s["obs_off"][q + 1]):
            if (int(s["obs_kf"][j]), q) not in erased:
                okf.append(s["obs_kf"][j])
                oidx.append(s["obs_idx"][j])
        off.append(len(okf))
    assert 0 < len(erased) and len(okf) == len(s["obs_kf"]) - len(erased)
    lists = [upload(np.array(a, np.int32), PAD, PAD) for a in (off, okf, oidx, np.zeros(n_pts, np.int32))]
    row = upload(s["row"], PAD, PAD)
    cols = dict(normal=Guarded(np.full((s["n_rows"], 3), -7.0, np.float32)), max_d=Guarded(np.full(s["n_rows"], -7.0, np.float32)),
                min_d=Guarded(np.full(s["n_rows"], -7.0, np.float32)))
    status = Guarded.cells(1)
    torch.cuda.synchronize()
    ctx.enqueue_update_map_points(c.dirs.ptr, n_kfs, n_pts, row[1], s["n_rows"], lists[0][1], lists[1][1], lists[2][1], len(okf), lists[3][1],
                                  api.MP_NORMAL_DEPTH, c.pos.ptr, cols["normal"].ptr, cols["max_d"].ptr, cols["min_d"].ptr, 0, 0, status.ptr,
                                  stream=st.cuda_stream)
    st.synchronize()
    assert int(status.fetch()[0]) == 0
    scale, Ow = ctx.tables()["scale"], got["dirs"]["Ow"]
    normal, max_d, min_d = cols["normal"].fetch(), cols["max_d"].fetch(), cols["min_d"].fetch()
    checked = 0
    for q in range(n_pts):
        r, lst = int(s["row"][q]), list(range(off[q], off[q + 1]))
        if not lst:
            assert normal[r, 0] == -7.0 and max_d[r] == -7.0
            continue
        level = int(s["kfs"][okf[lst[0]]][0]["octave"][oidx[lst[0]]])
        nrm, mx, mn = MP.update_normal_and_depth(got["pos"][r], [Ow[okf[j]] for j in lst], 0, level, scale, S.NLEVELS)
        assert np.array(nrm, np.float32).tobytes() == normal[r].tobytes() and mx == max_d[r] and mn == min_d[r], q
        checked += 1
    assert checked >= 35
