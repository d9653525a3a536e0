"""orbfe_enqueue_optimize_sim3 / orbfe_optimize_sim3 (Optimizer::OptimizeSim3, reference src/Optimizer.cc:1090-1285;
orbslam2_amd/csrc/orbfe_sim3_opt.hip) against the float64 model (tests/sim3_opt_model.py) on the scenes of tests/sim3_opt_scenes.py, which
tests/test_sim3_opt_model.py has checked on the CPU: every scene keeps 1 % distance from th2 at both classifications, so n_inliers,
d_match12 and d_status are compared EXACTLY and no entry is left out.  d_S12 is compared as the rotation matrix of its quaternion, t and
s within SIM3_ATOL.

SIM3_ATOL -- measured, as the issue of this feature prescribes: the largest |device - model| over all scenes of this file on the MI355X
was  8.2e-08  (scene early with min_inliers = 8, whose second optimize() runs on 8 correspondences; the 40-correspondence scenes reach
4.1e-08; entries of R, t in metres, s);  SIM3_ATOL = 8 x 8.2e-08 = 6.6e-07, rounded up to one digit: 7e-07.
That size is the numeric Jacobian's: J carries a relative noise of 1e-6, so the zero of b = J^T W e that the solver finds moves by
(noise of b) / H -- 1e-10 in the rotation, 1e-8 m in the translation -- between two correct implementations of the same arithmetic.
The factor covers the spread the header of tests/test_pose.py documents: the solver's stop rules compare nearly equal chi2 values, and where the model ran k trials the device may
run k +- 1 tiny ones.  The model returns its iteration and trial counts; a difference above the pose call's 1e-5 would mean a decision
flipped that matters, and is not to be accepted.

Shapes are the smallest that reach each path (96 and 80 keypoint slots, 40 correspondences; 12 for the early return; one keyframe of
more slots than ORBFE_SIM3_OPT_LDS_SLOTS for the table in HBM).  Device arrays and guards follow tests/device_arrays.py: inputs between
PAD readable entries, outputs between sentinel rows, never the default stream.
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import sim3_opt_model as M
from tests import sim3_opt_scenes as S
from tests.device_arrays import Guarded, context, upload

HERE = os.path.dirname(os.path.abspath(__file__))
PAD = 64
SIM3_ATOL = 7e-7   # see the header: 8 x the measured 8.2e-08, rounded up to one digit
POSE_ATOL = 1e-5   # tests/test_pose.py: the ceiling SIM3_ATOL may not exceed


@pytest.fixture(scope="module")
def gpu():
    import torch
    from orbslam2_amd import api
    ctx = context(api)
    assert np.array_equal(ctx.tables()["inv_sigma2"][:S.NLEVELS], S.INV_SIGMA2)
    assert api.SIM3_OPT_LDS_SLOTS == S.LDS_SLOTS
    yield api, ctx, torch.cuda.Stream()
    ctx.close()


class _Call:
    """One scene in HBM: inputs uploaded once, fresh guarded outputs."""

    def __init__(self, api, s):
        self.s = s
        n1, n2 = len(s["keys1"]), len(s["keys2"])
        self.own = []

        def up(a):
            if len(a) == 0:
                return 0                                  # the library is to see NULL under n == 0
            t, p = upload(a, front=PAD, pad=PAD)
            self.own.append(t)
            return p
        self.kf1, self.kf2 = api.GridKeyframe(), api.GridKeyframe()
        self.kf1.keys_un, self.kf1.n = up(s["keys1"]) or None, n1
        self.kf2.keys_un, self.kf2.n = up(s["keys2"]) or None, n2
        self.pos1, self.pos2, self.valid1, self.valid2 = up(s["pos1"]), up(s["pos2"]), up(s["valid1"]), up(s["valid2"])
        self.prior = 0 if s["prior12"] is None else up(s["prior12"])
        self.match = Guarded(s["match12"] if n1 else np.zeros(0, np.int32), guard_rows=PAD) if n1 else None
        self.S12 = Guarded(np.full(8, np.nan))
        self.n_in, self.status = Guarded.cells(1), Guarded.cells(1)

    def enqueue(self, ctx, st, params=None):
        s = self.s
        ctx.enqueue_optimize_sim3(self.kf1, s["T1w"], self.pos1, self.valid1, self.kf2, s["T2w"], self.pos2, self.valid2, s["s12"], s["R12"], s["t12"],
                                  s["th2"], s["fix_scale"], self.match.ptr if self.match else 0, self.S12.ptr, self.n_in.ptr, self.status.ptr,
                                  d_prior12=self.prior, params=params, stream=st.cuda_stream)

    def fetch(self):
        return dict(S12=self.S12.fetch(), match12=self.match.fetch() if self.match else np.zeros(0, np.int32), n_inliers=int(self.n_in.fetch()[0]),
                    status=int(self.status.fetch()[0]))


def _s12_diff(a, b):
    return max(np.abs(M.quat_matrix(a[:4]) - M.quat_matrix(b[:4])).max(), np.abs(a[4:8] - b[4:8]).max())


def _compare(name, got, ref):
    d = _s12_diff(got["S12"], ref["S12"])
    print("%-15s n_corr %3d inliers %3d status %2d  model iterations %s trials %s  |S12 - model| %.3e" % (
        name, ref["n_corr"], got["n_inliers"], got["status"], ref["iterations"], ref["trials"], d))
    assert got["status"] == ref["status"], name
    assert got["n_inliers"] == ref["n_inliers"], name
    assert np.array_equal(got["match12"], ref["match12"]), (name, np.nonzero(got["match12"] != ref["match12"])[0][:8])
    assert d <= SIM3_ATOL <= POSE_ATOL, (name, d)
    return d


def _same_bits(a, b):
    return (a["S12"].tobytes() == b["S12"].tobytes() and np.array_equal(a["match12"], b["match12"]) and a["n_inliers"] == b["n_inliers"]
            and a["status"] == b["status"])


def _alone(gpu, name, params=None):
    api, ctx, st = gpu
    c = _Call(api, S.scene(name))
    c.enqueue(ctx, st, params)
    st.synchronize()
    return c.fetch()


@pytest.mark.gpu
@pytest.mark.parametrize("name", S.DEVICE_SCENES)
def test_gpu_scene_against_the_model(gpu, name):
    """clean: the more_iterations_clean path; outliers: more_iterations_outliers with flags; fix_scale; early: the early return; none /
    kf1_empty: no correspondence; prior: d_prior12 merged on the device; invalid_slots: valid = 0 on either side; bad_*: d_status with
    the other rows unharmed; scratch_table: the table in HBM."""
    s, ref = S.scene(name), S.model(name)
    got = _alone(gpu, name)
    _compare(name, got, ref)
    if name in ("early", "none", "kf1_empty"):      # the input Sim3, bit for bit
        assert got["n_inliers"] == 0 and np.array_equal(got["S12"], ref["S12"])
    if name == "fix_scale":
        assert got["S12"][7] == float(s["s12"])     # exactly
    if name == "invalid_slots":
        held = s["slots1"][[3, 7, 20]]
        assert np.array_equal(got["match12"][held], s["match12"][held])
    if name == "prior":
        merged = np.where(s["prior12"] >= 0, s["prior12"], s["match12"])
        kept = got["match12"] >= 0
        assert np.array_equal(got["match12"][kept], merged[kept]) and kept[s["prior12"] >= 0].any()
    if name.startswith("bad_"):
        assert got["status"] == M.ERR_INVALID and got["n_inliers"] == 39


@pytest.mark.gpu
def test_gpu_iteration_parameters_are_honoured(gpu):
    """Other iteration counts and another inlier floor than the reference's: the model takes the same parameters."""
    api, ctx, st = gpu
    for name, prm in (("outliers", (2, 3, 2, 5)), ("early", (5, 10, 5, 8)), ("clean", (1, 1, 1, 41))):
        ref = S.run_model(S.scene(name), params=prm)
        got = _alone(gpu, name, api.Sim3OptParams(*prm))
        _compare("%s %s" % (name, prm), got, ref)
    assert S.run_model(S.scene("early"), params=(5, 10, 5, 8))["n_inliers"] == 8      # 12 - 4 reaches a floor of 8 ...
    assert S.run_model(S.scene("clean"), params=(1, 1, 1, 41))["n_inliers"] == 0      # ... and 40 clean ones miss one of 41


@pytest.mark.gpu
def test_gpu_host_entry_point_equals_the_enqueue_form_bit_for_bit(gpu):
    api, ctx, st = gpu
    for name in ("outliers", "prior", "fix_scale", "early", "kf1_empty", "scratch_table"):
        s = S.scene(name)
        dev = _alone(gpu, name)
        S12, m, n = ctx.optimize_sim3(s["keys1"], s["T1w"], s["pos1"], s["valid1"], s["keys2"], s["T2w"], s["pos2"], s["valid2"], s["s12"], s["R12"], s["t12"],
                                      s["th2"], s["fix_scale"], s["match12"], prior12=s["prior12"])
        assert _same_bits(dev, dict(S12=S12, match12=m, n_inliers=n, status=0)), name
    s = S.scene("kf1_empty")                        # keyframe 2 empty as well: every padded array of the call is empty; still the input Sim3
    S12, m, n = ctx.optimize_sim3(s["keys1"], s["T1w"], s["pos1"], s["valid1"], s["keys2"][:0], s["T2w"], s["pos2"][:0], s["valid2"][:0], s["s12"], s["R12"], s["t12"],
                                  s["th2"], s["fix_scale"], s["match12"], prior12=s["prior12"])
    assert len(s["keys1"]) == 0 and _same_bits(_alone(gpu, "kf1_empty"), dict(S12=S12, match12=m, n_inliers=n, status=0)), "both empty"
    s = S.scene("bad_octave1")                      # what only the device sees comes back as the call's error
    with pytest.raises(api.OrbfeError) as e:
        ctx.optimize_sim3(s["keys1"], s["T1w"], s["pos1"], s["valid1"], s["keys2"], s["T2w"], s["pos2"], s["valid2"], s["s12"], s["R12"], s["t12"], s["th2"], 0,
                          s["match12"])
    assert e.value.code == api.ERR_INVALID


@pytest.mark.gpu
def test_gpu_calls_queued_on_one_stream_equal_each_alone(gpu):
    """The scratch (the HBM table) and the LDS are the call's own for its duration: queued back to back without a host wait, every
    call gives the bits it gives alone."""
    api, ctx, st = gpu
    names = ["scratch_table", "outliers", "fix_scale", "scratch_table", "prior"]
    alone = {n: _alone(gpu, n) for n in set(names)}
    calls = [_Call(api, S.scene(n)) for n in names]
    for c in calls:
        c.enqueue(ctx, st)
    st.synchronize()
    for n, c in zip(names, calls):
        assert _same_bits(c.fetch(), alone[n]), n
    assert _same_bits(_alone(gpu, "outliers"), alone["outliers"])   # and run to run


@pytest.mark.gpu
def test_gpu_optimizer_header_wrapper(gpu):
    """ORB_SLAM2::Optimizer::OptimizeSim3 of orbslam2_amd/host/Optimizer.h (through tests/sim3_blocks/optimizer_wrapper.cpp) is a thin
    call of orbfe_optimize_sim3: the same bits."""
    api, ctx, st = gpu
    path = os.path.join(HERE, "sim3_blocks", "libsim3_wrapper.so")
    if not os.path.exists(path):
        raise RuntimeError("tests/sim3_blocks/libsim3_wrapper.so is missing: __graft_entry__.build() compiles it")
    W = C.CDLL(path)
    vp = C.c_void_p
    W.sim3_wrapper_optimize.restype = C.c_int
    W.sim3_wrapper_optimize.argtypes = [vp] + [vp, C.c_int, vp, vp, vp] * 2 + [C.c_float, vp, vp, vp, vp, vp, C.c_float, C.c_int, C.POINTER(C.c_int)]
    for name in ("outliers", "prior"):
        s = S.scene(name)
        m = s["match12"].copy(); S12 = np.zeros(8); n = C.c_int()
        p = lambda a: np.ascontiguousarray(a).ctypes.data_as(vp)
        keep = [np.ascontiguousarray(s[k]) for k in ("keys1", "T1w", "pos1", "valid1", "keys2", "T2w", "pos2", "valid2", "R12", "t12")]
        pr = None if s["prior12"] is None else np.ascontiguousarray(s["prior12"])
        rc = W.sim3_wrapper_optimize(ctx.h, p(keep[0]), len(keep[0]), p(keep[1]), p(keep[2]), p(keep[3]), p(keep[4]), len(keep[4]), p(keep[5]), p(keep[6]),
                                     p(keep[7]), float(s["s12"]), p(keep[8]), p(keep[9]), p(m), None if pr is None else p(pr), p(S12), s["th2"],
                                     s["fix_scale"], C.byref(n))
        assert rc == 0
        assert _same_bits(dict(S12=S12, match12=m, n_inliers=n.value, status=0), _alone(gpu, name)), name
    s = S.scene("bad_match_high")                   # the wrapper throws on the library's error
    m = s["match12"].copy(); S12 = np.zeros(8); n = C.c_int()
    keep = [np.ascontiguousarray(s[k]) for k in ("keys1", "T1w", "pos1", "valid1", "keys2", "T2w", "pos2", "valid2", "R12", "t12")]
    p = lambda a: a.ctypes.data_as(vp)
    assert W.sim3_wrapper_optimize(ctx.h, p(keep[0]), len(keep[0]), p(keep[1]), p(keep[2]), p(keep[3]), p(keep[4]), len(keep[4]), p(keep[5]), p(keep[6]),
                                   p(keep[7]), float(s["s12"]), p(keep[8]), p(keep[9]), p(m), None, p(S12), s["th2"], 0, C.byref(n)) == -100


@pytest.mark.gpu
def test_gpu_bad_arguments_are_refused_and_queue_nothing(gpu):
    api, ctx, st = gpu
    s = S.scene("clean")
    c = _Call(api, s)

    def refused(**kw):
        a = dict(kf1=c.kf1, pos1=c.pos1, valid1=c.valid1, kf2=c.kf2, pos2=c.pos2, valid2=c.valid2, th2=s["th2"], match=c.match.ptr, S12=c.S12.ptr,
                 n_in=c.n_in.ptr, status=c.status.ptr, params=None)
        a.update(kw)
        with pytest.raises(api.OrbfeError) as e:
            ctx.enqueue_optimize_sim3(a["kf1"], s["T1w"], a["pos1"], a["valid1"], a["kf2"], s["T2w"], a["pos2"], a["valid2"], s["s12"], s["R12"], s["t12"],
                                      a["th2"], 0, a["match"], a["S12"], a["n_in"], a["status"], params=a["params"], stream=st.cuda_stream)
        assert e.value.code == api.ERR_INVALID, kw
    big = api.GridKeyframe(); big.keys_un, big.n = c.kf1.keys_un, 65536
    neg = api.GridKeyframe(); neg.keys_un, neg.n = c.kf2.keys_un, -1
    nokeys = api.GridKeyframe(); nokeys.n = c.kf1.n
    for kw in (dict(th2=0.0), dict(th2=-1.0), dict(kf1=big), dict(kf2=neg), dict(kf1=nokeys), dict(pos1=0), dict(valid2=0), dict(match=0), dict(S12=0),
               dict(n_in=0), dict(status=0), dict(params=api.Sim3OptParams(0, 10, 5, 10)), dict(params=api.Sim3OptParams(5, 0, 5, 10)),
               dict(params=api.Sim3OptParams(5, 10, 0, 10)), dict(params=api.Sim3OptParams(5, 10, 5, 0))):
        refused(**kw)
    st.synchronize()
    assert c.match.untouched() and c.S12.untouched() and c.n_in.untouched() and c.status.untouched()
