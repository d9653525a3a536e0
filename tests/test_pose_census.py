"""A census of the PoseOptimization solver's branches, on the oracle and on the kernel, and non-finite input.

CPU: every scene of tests/pose_scenes.py meets the three conditions that make the GPU comparison at test_pose.POSE_ATOL meaningful
(classification margin, insensitivity to the order of the edges, |t| < 1 m), and the union of the oracle's traces over them -- kept
in tests/golden/pose_census.json -- shows every branch that honest input reaches: the four quaternion branches of the input pose,
all 15 pivot exchanges of the LDLT, rejected trials, the stop rules, a round with no active edge, ne < 10 and ne < 3, the
small-angle exponential, Huber edges on both sides of delta^2, an outlier that returns, a round that ends on a rejected trial.

GPU: the same scenes through the host entry point (edge table in LDS), through orbfe_enqueue_pose_optimization with a bound of
4097 slots (edge table in HBM) and as batches, with test_pose._compare's assertions: flags equal, count equal, pose within
POSE_ATOL.  Then one poisoned slot (a map point on the camera plane, a NaN or an inf coordinate): the call returns, the
neighbours of the poisoned problem are untouched, and the poisoned problem itself follows the oracle.
"""
import json
import os

import numpy as np
import pytest

from tests import pose_scenes as PS
from tests.test_pose import POSE_ATOL

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_census.json")

_ORACLE = {}


def oracle_runs():
    """(T, outlier, n, trace) of the oracle for every scene, computed once."""
    if not _ORACLE:
        for name, s in PS.scenes().items():
            _ORACLE[name] = (s, PS.run_oracle(s))
    return _ORACLE


# ---------------------------------------------------------------- CPU

def test_scenes_meet_the_three_conditions():
    for name, (s, (T, out, n, tr)) in oracle_runs().items():
        assert 12 <= len(s["keys"]) <= 300, name
        if tr["ne"] >= 3:
            assert tr["min_margin"] >= 1e-4, (name, tr["min_margin"])         # no classification within 1e-4 of its threshold
        for p in range(3):                                                    # a permutation changes the summation order as the kernel's tree does
            order = np.random.default_rng(500 + p).permutation(len(s["keys"]))
            T2, out2, n2, _ = PS.run_oracle(s, order=order)
            assert n2 == n and np.array_equal(out2, out), (name, p)
            assert np.abs(T2 - T).max() <= 2.5e-6, (name, p, np.abs(T2 - T).max())   # a quarter of POSE_ATOL
        assert np.abs(T[:3, 3]).max() < 1.0 and np.abs(s["T0"][:3, 3]).max() < 1.0, name   # POSE_ATOL keeps its meaning
        assert np.isfinite(T).all(), name


def test_census_shows_every_required_branch():
    got = PS.census()
    with open(GOLDEN) as f:
        want = json.load(f)
    assert got == want, "tests/golden/pose_census.json no longer matches the oracle's traces (regenerate it with pose_scenes.census())"
    for item in PS.REQUIRED:
        assert want["union"][item] >= 1, item
    assert set(want["union"]) == set(PS.REQUIRED + PS.RECORDED)


def test_trace_counts_are_consistent():
    for name, (s, (T, out, n, tr)) in oracle_runs().items():
        assert tr["ne"] == int(s["has"].sum()), name
        assert tr["accepted"] + tr["rejected"] == tr["solves"], name
        assert tr["rounds"] == (0 if tr["ne"] < 3 else 1 if tr["ne"] < 10 else 4), name
        assert all(k < c for k, c in tr["exchanges"]) and tr["qmax_max"] <= 10, name


# ---------------------------------------------------------------- GPU

def _ctx(cam):
    from orbslam2_amd import api
    return api.Context(width=1241, height=376, nfeatures=2000, max_images=1, **PS.CAMS[cam])


def _same_as_oracle(got, ref, what):
    """test_pose._compare's assertions."""
    (Tg, outg, ng), (Tr, outr, nr) = got, ref[:3]
    assert ng == nr, (what, ng, nr)
    assert np.array_equal(outg, outr), (what, np.nonzero(outg != outr)[0][:10])
    assert np.abs(Tg - Tr).max() <= POSE_ATOL, (what, np.abs(Tg - Tr).max())


def _cat(ss):
    off = np.cumsum([0] + [len(s["keys"]) for s in ss]).astype(np.int32)
    cat = {k: np.ascontiguousarray(np.concatenate([s[k] for s in ss])) for k in ("keys", "ur", "has", "Xw")}
    return off, cat, np.stack([s["T0"] for s in ss])


def _enqueue(ctx, ss, bound, fill=9):
    """orbfe_enqueue_pose_optimization on device-resident arrays; outlier pre-filled with `fill`.  Returns (T, outlier, n)."""
    import torch
    off, cat, T0 = _cat(ss)
    dev = torch.device("cuda:0")
    d = {k: torch.from_numpy(v.view(np.uint8).reshape(-1) if v.dtype.fields else v).to(dev) for k, v in cat.items()}
    d_off, d_T = torch.from_numpy(off).to(dev), torch.from_numpy(T0).to(dev)
    d_out = torch.full((max(int(off[-1]), 1),), fill, dtype=torch.uint8, device=dev)
    d_n = torch.zeros(len(ss), dtype=torch.int32, device=dev)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    ctx._check(ctx.L.orbfe_enqueue_pose_optimization(ctx.h, len(ss), d_off.data_ptr(), d["keys"].data_ptr(), d["ur"].data_ptr(), d["has"].data_ptr(),
                                                     d["Xw"].data_ptr(), d_T.data_ptr(), d_out.data_ptr(), d_n.data_ptr(), bound, st.cuda_stream))
    st.synchronize()
    return d_T.cpu().numpy(), d_out.cpu().numpy()[: int(off[-1])], d_n.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("cam", range(len(PS.CAMS)))
def test_gpu_census_scenes_match_oracle_on_both_kernel_variants(cam):
    runs = {k: v for k, v in oracle_runs().items() if v[0]["cam"] == cam}
    assert runs
    ctx = _ctx(cam)
    single = {}
    for name, (s, ref) in runs.items():
        got = ctx.pose_optimization(s["T0"], s["keys"], s["ur"], s["has"], s["Xw"])
        _same_as_oracle(got, ref, (name, "lds"))
        single[name] = got
        Th, outh, nh = _enqueue(ctx, [s], 4097, fill=0)
        _same_as_oracle((Th[0], outh, int(nh[0])), ref, (name, "hbm"))
    # one batch of all scenes of this camera against the single runs, bit for bit
    names = list(runs)
    off, cat, T0 = _cat([runs[k][0] for k in names])
    Tb, outb, nb = ctx.pose_optimization_batch(T0, off, cat["keys"], cat["ur"], cat["has"], cat["Xw"])
    for k, name in enumerate(names):
        Tg, outg, ng = single[name]
        assert np.array_equal(Tb[k], Tg) and nb[k] == ng and np.array_equal(outb[off[k]:off[k + 1]], outg), name
    ctx.close()


def poisoned(kind):
    """A 64-slot problem started at the identity whose slot 20 is poisoned."""
    s = PS.make(seed=300, n=64, has_frac=0.8, rv=(0.002, -0.001, 0.001), t=(0.01, -0.005, -0.02))   # the identity is 2 cm off the truth
    s["has"][20] = 1
    s["has"][[5, 40]] = 0
    if kind == "z0":
        s["Xw"][20, 2] = 0.0          # on the camera plane of the start pose: 1 / z = inf
    elif kind == "nan":
        s["Xw"][20, 1] = np.nan
    else:
        s["Xw"][20, 0] = np.inf
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["z0", "nan", "inf"])
def test_gpu_non_finite_input_follows_the_oracle_and_spares_its_neighbours(kind):
    """The oracle's LDLT writes 0 where a pivot is not above DBL_MIN (NaN included), so a system poisoned by one slot gives a
    zero step: every trial equals the estimate, the pose comes back unchanged and the classification sees the start pose.
    (Measured on the oracle, NaN coordinate: 80 evaluations, pose unchanged.)  Eigen's own NaN behaviour is unpinned like the
    rest of the oracle, DESIGN.md section 2."""
    bad = poisoned(kind)
    left, right = PS.make(seed=301, n=100), PS.make(seed=302, n=33)
    pre = np.full(64, 7, np.uint8)
    Tr, outr, nr, tr = PS.run_oracle(bad, outlier=pre)
    assert np.isfinite(Tr).all()
    ctx = _ctx(0)
    # alone, LDS edge table
    got = ctx.pose_optimization(bad["T0"], bad["keys"], bad["ur"], bad["has"], bad["Xw"], pre)
    assert (got[1][bad["has"] == 0] == 7).all()               # bytes without a map point keep the caller's value
    _same_as_oracle(got, (Tr, outr, nr), (kind, "lds alone"))
    # alone, HBM edge table
    Th, outh, nh = _enqueue(ctx, [bad], 4097, fill=7)
    assert (outh[bad["has"] == 0] == 7).all()
    _same_as_oracle((Th[0], outh, int(nh[0])), (Tr, outr, nr), (kind, "hbm alone"))
    # the middle problem of a batch of three, both variants: the neighbours equal their single runs bit for bit
    trio = [left, bad, right]
    off, cat, T0 = _cat(trio)
    fill = np.full(int(off[-1]), 7, np.uint8)
    Tb, outb, nb = ctx.pose_optimization_batch(T0, off, cat["keys"], cat["ur"], cat["has"], cat["Xw"], fill)
    Te, oute, ne = _enqueue(ctx, trio, 4097, fill=7)
    for k in (0, 2):
        s = trio[k]
        Tg, outg, ng = ctx.pose_optimization(s["T0"], s["keys"], s["ur"], s["has"], s["Xw"], np.full(len(s["keys"]), 7, np.uint8))
        assert np.array_equal(Tb[k], Tg) and nb[k] == ng and np.array_equal(outb[off[k]:off[k + 1]], outg), (kind, k, "lds")
        T1, out1, n1 = _enqueue(ctx, [s], 4097, fill=7)
        assert np.array_equal(Te[k], T1[0]) and ne[k] == n1[0] and np.array_equal(oute[off[k]:off[k + 1]], out1), (kind, k, "hbm")
        assert ng >= 10
    _same_as_oracle((Tb[1], outb[off[1]:off[2]], int(nb[1])), (Tr, outr, nr), (kind, "lds batch"))
    _same_as_oracle((Te[1], oute[off[1]:off[2]], int(ne[1])), (Tr, outr, nr), (kind, "hbm batch"))
    assert (outb[off[1]:off[2]][bad["has"] == 0] == 7).all() and (oute[off[1]:off[2]][bad["has"] == 0] == 7).all()
    ctx.close()
