"""orbfe_enqueue_optimize_essential_graph / orbfe_optimize_essential_graph (Optimizer::OptimizeEssentialGraph, reference
src/Optimizer.cc:825-1088; orbslam2_amd/csrc/orbfe_essential_graph.hip) against the float64 model (tests/essential_graph_model.py, proved
by tests/test_essential_graph_model.py) on the scenes of tests/essential_graph_scenes.py.

Scenes: two (one edge), chain3, ring6 and ring6_fix_scale (a drifted ring closed by corrected Sim3s of scale 1.1 on the current keyframe
and two neighbours), covis40 / covis40_fix_scale (40 keyframes with covisibility edges: the workspace in the LDS), hbm300 (300 keyframes:
the workspace in HBM), dup_rev (duplicate and reversed edges), the boundary scenes of the kernel's strides (EG_THREADS = 256: kfs_255 /
256 / 257 for the loops over keyframes, kfs_17 / 18 for keyframes x 15, kfs_37 / 38 for free keyframes x 7, edges_255 / 256 / 257; the
slot loops (slots x 49) and the update loops (updates x 49 + rows x 7) cross 256 inside ring6 and covis40), no_points, and faulty (three
edges with faulty indices, a NaN in one corrected Sim3, two points whose keyframe lies outside the map).

Exact: iterations, trials, the number of edges that take part, the codes and the status against the model; the recovery (Tcw, Ow) and the
point correction against the model fed the DEVICE's final Sim3s (these stages call no libm: bit for bit); two calls on one stream, the
synchronous form and the host wrapper against each other.

Tolerance: the final Sim3s as R (the entries of toRotationMatrix), t and s against the model's.  Each bound is 8 x the largest
|device - model| over all scenes of this file on the MI355X, rounded up to one digit (DESIGN.md section 4s has both columns):
    quantity      largest difference      bound
    R entries     2.344e-07 (kfs_38)      R_ATOL = 2e-6
    t (metres)    4.109e-07 (dup_rev)     T_ATOL = 4e-6
    s             4.092e-08 (covis40)     S_ATOL = 4e-7
The differences are the numeric Jacobians' own noise (both sides divide rounding by 2e-9; two libms differ by 7e-9 in an entry) times the
graph's conditioning: 1e-12 after the first iteration of a 256-keyframe chain, 1e-7 after two or three iterations of 40 keyframes.  hbm300
runs ONE iteration for that reason: with three, device and model agree in every decision (3 iterations, 3 trials, lambda to 3e-5) and
differ by 5.6e-5 in R and 2.2e-4 in t, which is what the model alone moves by under 7e-9 of Jacobian noise (3.3e-4).
None may exceed the pose call's 1e-5 (tests/test_pose.py): a larger difference would mean a flipped stop-rule decision, to be found
through the iteration and trial counts, not accepted.

Device arrays and guards follow tests/device_arrays.py: inputs between PAD readable entries, every output between sentinel rows and
started from a sentinel value, never the default stream.
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import essential_graph_model as M
from tests import essential_graph_scenes as SC
from tests import sim3_opt_model as S3
from tests.device_arrays import Guarded, context, upload

PAD = 64
R_ATOL = 2e-6       # see the header: 8 x the measured maxima, rounded up to one digit
T_ATOL = 4e-6
S_ATOL = 4e-7
CEILING = 1e-5      # tests/test_pose.py
HERE = os.path.dirname(os.path.abspath(__file__))

_MODEL = {}


def model(name):
    """The model's result of a scene, computed once and shared."""
    if name not in _MODEL:
        _MODEL[name] = M.run(**SC.scene(name))
    return _MODEL[name]


@pytest.fixture(scope="module")
def gpu():
    import torch
    from orbslam2_amd import api
    ctx = context(api)
    assert api.EG_LAMBDA_INIT == M.LAMBDA_INIT
    yield api, ctx, torch.cuda.Stream()
    ctx.close()


class _Call:
    """One scene in HBM: inputs uploaded once, fresh guarded outputs."""

    def __init__(self, api, s, plan=None, obs_kfs=True):
        import torch
        self.s, self.own = s, []
        n_kfs, n_edges, n_pts = len(s["Tcw"]), len(s["edge_i"]), len(s["pos"])

        def up(a):
            t, p = upload(a, front=PAD, pad=PAD)
            self.own.append(t)
            return p
        self.blob = api.essential_graph_plan(n_kfs, s["fixed_kf"], s["edge_i"], s["edge_j"])
        self.plan = up(self.blob if plan is None else plan)
        self.corr, self.hc, self.nonc, self.hn = up(s["corrected"]), up(s["has_corrected"]), up(s["noncorrected"]), up(s["has_noncorrected"])
        self.ei, self.ej, self.ek = up(s["edge_i"]), up(s["edge_j"]), up(s["edge_kind"])
        self.ref, self.valid = (up(s["pt_ref"]), up(s["pt_valid"])) if n_pts else (0, 0)
        self.Tcw = Guarded(s["Tcw"])
        self.pos = Guarded(s["pos"]) if n_pts else None
        dirs = np.zeros(n_kfs, api.OBS_KF_DTYPE)
        dirs["desc"], dirs["keys_un"], dirs["n"], dirs["bad"], dirs["reserved"] = 0x1111, 0x2222, 77, 5, 9
        dirs["Ow"] = np.arange(3 * n_kfs, dtype=np.float32).reshape(n_kfs, 3) + 1000
        self.dirs0 = dirs
        self.dirs = Guarded(dirs) if obs_kfs else None
        self.ecode = Guarded(np.full(n_edges, 0xEE, np.uint8), guard_rows=PAD)
        self.pcode = Guarded(np.full(max(n_pts, 1), 0xEE, np.uint8), guard_rows=PAD)
        self.sim3 = Guarded(np.full((n_kfs, 8), -7.0))
        self.status = Guarded.cells(1)
        self.info = Guarded(np.frombuffer(bytes([0xEE]) * 48, api.EG_INFO_DTYPE).copy())
        torch.cuda.synchronize()   # the uploads and fills above ran on torch's own stream

    def enqueue(self, ctx, st, header=None):
        s = self.s
        ctx.enqueue_optimize_essential_graph(len(s["Tcw"]), s["fixed_kf"], self.Tcw.ptr, self.corr, self.hc, self.nonc, self.hn, self.ei, self.ej, self.ek,
                                             len(s["edge_i"]), self.plan, self.blob if header is None else header, s["iterations"], s["fix_scale"],
                                             M.LAMBDA_INIT, self.pos.ptr if self.pos else 0, self.ref, self.valid, len(s["pos"]),
                                             self.dirs.ptr if self.dirs else 0, self.ecode.ptr, self.pcode.ptr, self.sim3.ptr, self.info.ptr, self.status.ptr,
                                             stream=st.cuda_stream)

    def fetch(self):
        return dict(Tcw=self.Tcw.fetch(), pos=self.pos.fetch() if self.pos else np.zeros((0, 3), np.float32), dirs=self.dirs.fetch() if self.dirs else None,
                    edge_code=self.ecode.fetch(), pt_code=self.pcode.fetch()[: len(self.s["pos"])], sim3=self.sim3.fetch(), info=self.info.fetch()[0],
                    status=int(self.status.fetch()[0]))

    def untouched(self):
        return all(g.untouched() for g in (self.Tcw, self.pos, self.dirs, self.ecode, self.pcode, self.sim3, self.info) if g is not None)


def _alone(gpu, name, **kw):
    api, ctx, st = gpu
    c = _Call(api, SC.scene(name), **kw)
    c.enqueue(ctx, st)
    st.synchronize()
    return c, c.fetch()


def _pose_differences(got, want, skip=()):
    dR = dt = ds = 0.0
    for v in range(len(want)):
        if v in skip:
            continue
        a, b = S3.unpack(got[v]), S3.unpack(want[v])
        dR = max(dR, float(np.abs(S3.quat_matrix(a[0]) - S3.quat_matrix(b[0])).max()))
        dt = max(dt, float(np.abs(np.array(a[1]) - np.array(b[1])).max()))
        ds = max(ds, abs(a[2] - b[2]))
    return dR, dt, ds


def _same(a, b):
    for k in ("Tcw", "pos", "edge_code", "pt_code", "sim3"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["info"].tobytes() == b["info"].tobytes() and a["status"] == b["status"]
    if a.get("dirs") is not None and b.get("dirs") is not None:
        assert a["dirs"].tobytes() == b["dirs"].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SC.SCENES))
def test_scene_against_the_model(gpu, name):
    api, ctx, st = gpu
    s = SC.scene(name)
    c, got = _alone(gpu, name)
    want = model(name)
    info, minfo = got["info"], want["info"]
    bad = [v for v in range(len(s["Tcw"])) if want["problem"].vbad[v]]
    dR, dt, ds = _pose_differences(got["sim3"], want["sim3"], bad)
    print("\n%s: device iterations %d trials %d chi2 %.9g -> %.9g lambda %.6g | model %d %d %.9g -> %.9g %.6g | dR %.3e dt %.3e ds %.3e | L blocks %d in_lds %d" % (
        name, info["iterations"], info["trials"], info["chi2_start"], info["chi2_end"], info["lambda_last"], minfo["iterations"], minfo["trials"],
        minfo["chi2_start"], minfo["chi2_end"], minfo["lambda_last"], dR, dt, ds, info["n_lblocks"], info["in_lds"]))
    # exact
    assert got["status"] == want["status"]
    assert np.array_equal(got["edge_code"], want["edge_code"]) and np.array_equal(got["pt_code"], want["pt_code"])
    assert (info["iterations"], info["trials"], info["n_active_edges"]) == (minfo["iterations"], minfo["trials"], minfo["n_active_edges"])
    hdr = np.frombuffer(c.blob[:20].tobytes(), api.ESSENTIAL_PLAN_HEADER_DTYPE)[0]
    assert info["n_lblocks"] == hdr["n_lblocks"]
    ws = (hdr["n_free"] + hdr["n_lblocks"]) * 49 + hdr["n_free"] * 7
    assert info["in_lds"] == (1 if ws <= api.EG_LDS_DOUBLES else 0)
    if name in ("covis40", "ring6"):
        assert info["in_lds"] == 1
    if name in ("hbm300", "kfs_256"):
        assert info["in_lds"] == 0
    # the recovery and the point kernel, bit for bit, from the device's own final Sim3s
    final = [S3.unpack(v) for v in got["sim3"]]
    T, Ow, pos, pcode = M.finish(want["problem"], final, s["Tcw"], s["pos"], s["pt_ref"], s["pt_valid"])
    assert got["Tcw"].tobytes() == T.tobytes()
    assert got["pos"].tobytes() == pos.tobytes()
    for v in range(len(T)):
        if v in bad:
            assert got["dirs"][v].tobytes() == c.dirs0[v].tobytes()
        else:
            assert got["dirs"]["Ow"][v].tobytes() == Ow[v].tobytes()
    for f in ("desc", "keys_un", "n", "bad", "reserved"):
        assert np.array_equal(got["dirs"][f], c.dirs0[f])
    invalid_pts = np.nonzero(np.asarray(s["pt_valid"]) == 0)[0]
    assert got["pos"][invalid_pts].tobytes() == np.asarray(s["pos"])[invalid_pts].tobytes()
    # tolerance
    rel = lambda a, b: abs(a - b) / max(abs(b), 1e-300)
    assert rel(info["chi2_start"], minfo["chi2_start"]) < 1e-9
    assert dR <= R_ATOL <= CEILING and dt <= T_ATOL <= CEILING and ds <= S_ATOL <= CEILING


@pytest.mark.gpu
def test_two_calls_on_one_stream_the_synchronous_form_and_the_wrapper_give_the_same_bits(gpu):
    api, ctx, st = gpu
    for name in ("ring6", "covis40_fix_scale", "faulty"):
        s = SC.scene(name)
        a, b = _Call(api, s), _Call(api, s)
        a.enqueue(ctx, st)
        b.enqueue(ctx, st)
        st.synchronize()
        ra, rb = a.fetch(), b.fetch()
        _same(ra, rb)
        sync = ctx.optimize_essential_graph(s["fixed_kf"], s["Tcw"], s["edge_i"], s["edge_j"], s["edge_kind"], s["corrected"], s["has_corrected"], s["noncorrected"],
                                            s["has_noncorrected"], s["iterations"], s["fix_scale"], M.LAMBDA_INIT, s["pos"], s["pt_ref"], s["pt_valid"])
        _same(dict(ra, dirs=None), dict(sync, dirs=None))
        ok = [v for v in range(len(s["Tcw"])) if np.all(np.isfinite(ra["sim3"][v]))]
        assert sync["Ow"][ok].tobytes() == ra["dirs"]["Ow"][ok].tobytes()
        # ORB_SLAM2::Optimizer::OptimizeEssentialGraph of orbslam2_amd/host/Optimizer.h
        L = C.CDLL(os.path.join(HERE, "essential_blocks", "libessential_wrapper.so"))
        L.eg_wrapper_optimize.restype = C.c_int
        L.eg_wrapper_optimize.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 7 + [C.c_int] * 3 + [C.c_void_p] * 5
        T, pos = np.ascontiguousarray(s["Tcw"], np.float32).copy(), np.ascontiguousarray(s["pos"], np.float32).copy()
        n_kfs, n_edges, n_pts = len(T), len(s["edge_i"]), len(pos)
        Ow, ecode, pcode, sim3 = np.zeros((n_kfs, 3), np.float32), np.zeros(n_edges, np.uint8), np.zeros(n_pts, np.uint8), np.zeros((n_kfs, 8))
        info, status = np.zeros(1, api.EG_INFO_DTYPE), np.zeros(1, np.int32)
        p = lambda x: np.ascontiguousarray(x).ctypes.data_as(C.c_void_p)
        keep = [np.ascontiguousarray(s[k]) for k in ("edge_i", "edge_j", "edge_kind", "corrected", "has_corrected", "noncorrected", "has_noncorrected", "pt_ref", "pt_valid")]
        rc = L.eg_wrapper_optimize(ctx.h, n_kfs, s["fixed_kf"], p(T), p(Ow), p(keep[0]), p(keep[1]), p(keep[2]), n_edges, p(keep[3]), p(keep[4]), p(keep[5]), p(keep[6]),
                                   p(pos), p(keep[7]), p(keep[8]), n_pts, int(s["fix_scale"]), s["iterations"], p(ecode), p(pcode), p(sim3), p(info), p(status))
        assert rc == 0
        _same(dict(sync, dirs=None), dict(Tcw=T.reshape(-1, 16), pos=pos, edge_code=ecode, pt_code=pcode, sim3=sim3, info=info[0], status=int(status[0]), dirs=None))
        assert Ow.tobytes() == sync["Ow"].tobytes()
    # no edge and no point: every padded array of the synchronous call is empty.  No vertex is active, so optimize() returns at once and
    # the poses come back re-derived from their quaternions (the 1e-6 of test_without_optional_tables_and_outputs)
    s, z = SC.scene("two"), np.zeros(0, np.int32)
    sync = ctx.optimize_essential_graph(0, s["Tcw"], z, z, np.zeros(0, np.uint8), iterations=2)
    want = M.run(s["Tcw"], 0, z, z, np.zeros(0, np.uint8), iterations=2)
    assert sync["status"] == 0 and [int(sync["info"][k]) for k in ("iterations", "trials", "n_active_edges")] == [0, 0, 0]
    assert len(sync["edge_code"]) == 0 and len(sync["pos"]) == 0 and len(sync["pt_code"]) == 0
    assert np.abs(sync["Tcw"] - want["Tcw"]).max() < 1e-6 and np.abs(sync["Tcw"] - s["Tcw"]).max() < 1e-6


@pytest.mark.gpu
def test_without_optional_tables_and_outputs(gpu):
    """No corrected / non-corrected table, no directory, no point codes, no Sim3 output: the poses come back as they went in (the
    measurements come from the initial estimates: zero error, x = 0), re-derived from their quaternions."""
    api, ctx, st = gpu
    s = SC.scene("ring6")
    c = _Call(api, s, obs_kfs=False)
    ctx.enqueue_optimize_essential_graph(6, 0, c.Tcw.ptr, 0, 0, 0, 0, c.ei, c.ej, c.ek, len(s["edge_i"]), c.plan, c.blob, 5, 0, M.LAMBDA_INIT, c.pos.ptr, c.ref, c.valid,
                                         len(s["pos"]), 0, c.ecode.ptr, 0, 0, c.info.ptr, c.status.ptr, stream=st.cuda_stream)
    st.synchronize()
    got = c.fetch()
    want = M.run(s["Tcw"], 0, s["edge_i"], s["edge_j"], s["edge_kind"], iterations=5, pos=s["pos"], pt_ref=s["pt_ref"], pt_valid=s["pt_valid"])
    assert got["status"] == 0 and not got["edge_code"].any() and c.sim3.untouched() and c.pcode.untouched()
    # zero up to the float32 rows (a quaternion that is a unit to 2^-24 only): the stop rules then act on rounding, the counts are not compared
    assert got["info"]["chi2_start"] < 1e-11 and want["info"]["chi2_start"] < 1e-11
    assert np.abs(got["Tcw"] - want["Tcw"]).max() < 1e-6 and np.abs(got["Tcw"] - s["Tcw"]).max() < 1e-6
    assert np.abs(got["pos"] - want["pos"]).max() < 1e-5


@pytest.mark.gpu
def test_a_mismatched_plan_writes_the_status_and_nothing_else(gpu):
    api, ctx, st = gpu
    s = SC.scene("ring6")
    other = SC.scene("dup_rev")
    other_blob = api.essential_graph_plan(len(other["Tcw"]), 0, other["edge_i"], other["edge_j"])
    flipped = api.essential_graph_plan(6, 0, s["edge_i"], s["edge_j"]).copy()
    flipped[0] ^= 1   # the magic
    moved = api.essential_graph_plan(6, 0, s["edge_i"], s["edge_j"]).copy()
    moved[10] += 1    # off_pos: a section that no longer follows the one before it
    stale = api.essential_graph_plan(6, 1, s["edge_i"], s["edge_j"])   # the plan of another fixed keyframe
    for plan, header in ((other_blob, None), (other_blob, other_blob), (flipped, None), (moved, None), (stale, None), (stale, stale)):
        c = _Call(api, s, plan=plan)
        c.enqueue(ctx, st, header=header)
        st.synchronize()
        assert int(c.status.fetch()[0]) == api.ERR_INVALID
        assert c.untouched()
    with pytest.raises(api.OrbfeError):
        c.enqueue(ctx, st, header=np.zeros(20, np.int32))   # not a plan header: refused on the host
    c = _Call(api, s)
    with pytest.raises(api.OrbfeError):
        ctx.enqueue_optimize_essential_graph(6, 6, c.Tcw.ptr, c.corr, c.hc, c.nonc, c.hn, c.ei, c.ej, c.ek, len(s["edge_i"]), c.plan, c.blob, 5, 0, M.LAMBDA_INIT,
                                             c.pos.ptr, c.ref, c.valid, len(s["pos"]), 0, c.ecode.ptr, 0, 0, c.info.ptr, c.status.ptr, stream=st.cuda_stream)
    with pytest.raises(api.OrbfeError):
        ctx.enqueue_optimize_essential_graph(6, 0, c.Tcw.ptr, c.corr, c.hc, c.nonc, c.hn, c.ei, c.ej, c.ek, len(s["edge_i"]), c.plan, c.blob, 5, 0, 0.0,
                                             c.pos.ptr, c.ref, c.valid, len(s["pos"]), 0, c.ecode.ptr, 0, 0, c.info.ptr, c.status.ptr, stream=st.cuda_stream)
    st.synchronize()
    assert c.untouched()


@pytest.mark.gpu
def test_faulty_input_leaves_the_rest_as_if_absent(gpu):
    """The faulty scene against the model of the same map WITHOUT the faulty edges: the same Sim3s up to the elimination order's rounding,
    and the keyframe with the NaN keeps its row, as do the points that refer to it."""
    api, ctx, st = gpu
    s = SC.scene("faulty")
    c, got = _alone(gpu, "faulty")
    assert got["status"] == api.ERR_INVALID
    assert got["edge_code"].tolist() == model("faulty")["edge_code"].tolist()
    assert got["edge_code"][-3:].tolist() == [api.EG_EDGE_INDEX] * 3 and set(got["edge_code"][:-3].tolist()) == {0, api.EG_EDGE_SIM3}
    touching6 = [(int(i) == 6 or int(j) == 6) for i, j in zip(s["edge_i"][:-3], s["edge_j"][:-3])]
    assert (got["edge_code"][:-3] == api.EG_EDGE_SIM3).tolist() == touching6
    assert got["pt_code"][:2].tolist() == [1, 1] and not got["pt_code"][2:].any()
    assert got["Tcw"][6].tobytes() == s["Tcw"][6].tobytes() and got["dirs"][6].tobytes() == c.dirs0[6].tobytes()
    for q in range(len(s["pos"])):
        if q < 2 or s["pt_ref"][q] == 6 or not s["pt_valid"][q]:
            assert got["pos"][q].tobytes() == s["pos"][q].tobytes()
    keep = [e for e in range(len(s["edge_i"])) if not got["edge_code"][e]]
    clean = M.run(s["Tcw"], 0, s["edge_i"][keep], s["edge_j"][keep], s["edge_kind"][keep], s["corrected"], s["has_corrected"], s["noncorrected"], s["has_noncorrected"],
                  iterations=s["iterations"], fix_scale=s["fix_scale"])
    dR, dt, ds = _pose_differences(got["sim3"], clean["sim3"], skip=(6,))
    assert dR <= R_ATOL and dt <= T_ATOL and ds <= S_ATOL
