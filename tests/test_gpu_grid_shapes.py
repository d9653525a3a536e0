"""Shapes at which a grid builder of ONE workgroup (grid_build_kernel: 1024 threads stride over the keypoints, LDS counters and
cursors) and a top-4 kept in registers (Top4, orbfe_match_window.hpp) can go wrong: frames of 1, 1023, 1025 and 3000 uploaded
keypoints, a cell crowded through duplicated coordinates (more than 1024 keypoints in it at n = 3000; below, the largest share
that n leaves room for: 1 / 600 / 600), keypoints outside the bounds (PosInGrid drops them), two that round to column 64
(dropped too, Q6), and windows with more than 256 statically admissible candidates whose prefix repeated map points use up.
Everything is compared with the oracle, exactly."""
import ctypes as C

import numpy as np
import pytest

from oracle import literal_matchers as LM
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FX, FY, CX, CY, BF = 500.0, 500.0, 320.0, 240.0, 50.0
W, H = 640, 480
BOUNDS = (0.0, float(W), 0.0, float(H))
CAM = O.Camera(FX, FY, CX, CY, BF, BF / FX)
CROWD_XY = np.array([(200.0, 150.0), (201.5, 151.0), (198.0, 152.25), (203.0, 148.0)], np.float32)  # all round to cell (20, 15)
CROWD_OCTAVE = 2
SIZES = (1, 1023, 1025, 3000)


def _frame(n):
    """n keypoints: first the crowd, then (room permitting) two on column 64 and three outside the bounds, the rest uniform."""
    rng = np.random.default_rng(1000 + n)
    n_crowd = {1: 1, 1023: 600, 1025: 600, 3000: 1100}[n]
    k = np.zeros(n, O.KP_DTYPE)
    k["x"] = rng.uniform(0, W - 5, n); k["y"] = rng.uniform(0, H - 6, n)
    k["octave"] = rng.integers(0, 8, n); k["angle"] = rng.uniform(0, 360, n); k["size"] = 31; k["class_id"] = -1
    base = rng.integers(0, 256, 32).astype(np.uint8)
    d = rng.integers(0, 256, (n, 32)).astype(np.uint8)
    crowd = rng.permutation(n)[:n_crowd]  # anywhere in the index range: the 1024-stride loop meets them in every round
    xy = CROWD_XY[rng.integers(0, len(CROWD_XY), n_crowd)]
    k["x"][crowd] = xy[:, 0]; k["y"][crowd] = xy[:, 1]; k["octave"][crowd] = CROWD_OCTAVE
    d[crowd] = base ^ np.packbits(rng.random((n_crowd, 256)) < 0.06, axis=1, bitorder="little")  # about 15 bits from the base
    if n > n_crowd + 5:
        rest = np.setdiff1d(np.arange(n), crowd)
        col64, outside = rest[[0, -1]], rest[[1, len(rest) // 2, -2]]
        k["x"][col64] = [637.0, 639.5]  # inside the image, PosInGrid rounds them to column 64
        k["x"][outside] = [-20.0, W + 1.5, 5.0]; k["y"][outside] = [10.0, 20.0, H + 30.0]
    has = (rng.random(n) < 0.1).astype(np.uint8)  # keypoints taken before the call, a tenth of the crowd among them
    return dict(n=n, k=k, d=d, ur=np.full(n, -1.0, np.float32), has=has, base=base, crowd=crowd)


@pytest.fixture(scope="module")
def ctx():
    from orbslam2_amd import api
    c = api.Context(width=W, height=H, fx=FX, fy=FY, cx=CX, cy=CY, bf=BF)
    yield c
    c.close()


@pytest.fixture(scope="module", params=SIZES)
def case(request):
    f = _frame(request.param)
    f["grid"] = O.Grid(f["k"], *BOUNDS)
    return f


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_grid_equals_the_oracle_cell_for_cell(ctx, case):
    n, k = case["n"], case["k"]
    off = np.zeros(64 * 48 + 1, np.int32); idx = np.zeros(n, np.int32)
    ctx.L.orbfe_assign_features_to_grid.restype = C.c_int
    ctx.L.orbfe_assign_features_to_grid.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert ctx.L.orbfe_assign_features_to_grid(ctx.h, C.byref(ctx._view(k, None, case["d"], BOUNDS)), _p(off), _p(idx)) == 0
    # oracle.Grid: a window over the whole grid lists its cells one after the other (cell x, cell y, insertion order)
    everything = case["grid"].features_in_area(W / 2, H / 2, 4.0 * W)
    assert off[-1] == len(everything) and idx[: off[-1]].tolist() == everything.tolist()
    # where one cell ends and the next begins: Frame::mGrid as the reference builds it
    lit = LM.Frame(k, None, None, BOUNDS, (FX, FY, CX, CY, BF, BF / FX), np.ones(8, np.float32))
    assert (np.diff(off) == np.array([[len(c) for c in col] for col in lit.mGrid]).ravel()).all()
    if n >= 1023:
        assert off[-1] == n - 5  # three outside the bounds, two on column 64
        assert off[20 * 48 + 15 + 1] - off[20 * 48 + 15] >= len(case["crowd"])
    assert n < 3000 or off[20 * 48 + 15 + 1] - off[20 * 48 + 15] > 1024


def test_window_over_the_crowded_cell(ctx, case):
    view = ctx._view(case["k"], None, case["d"], BOUNDS)
    for lo, hi in ((-1, -1), (CROWD_OCTAVE, CROWD_OCTAVE)):
        ref = case["grid"].features_in_area(200.0, 150.0, 12.0, lo, hi)
        assert ctx.features_in_area(view, 200.0, 150.0, 12.0, lo, hi).tolist() == ref.tolist()
        assert len(ref) >= len(case["crowd"])


def test_search_by_projection_last_in_windows_of_hundreds(ctx, case):
    """40 map points that project into the crowd, each 10 times and every match blocking its keypoint: 400 queries compete for the
    same keypoints, so the four-key prefix is used up at once and n_static (hundreds) sends the replay to the full list."""
    k, d, ur, has = case["k"], case["d"], case["ur"], case["has"]
    rng = np.random.default_rng(2000 + case["n"])
    m, rep = 40, 10
    u = rng.uniform(199.0, 202.0, m); v = rng.uniform(149.0, 152.0, m); z = rng.uniform(4.0, 20.0, m)
    pos = np.repeat(np.stack([(u - CX) * z / FX, (v - CY) * z / FY, z], axis=1).astype(np.float32), rep, axis=0)
    desc = np.repeat(case["base"][None] ^ np.packbits(rng.random((m, 256)) < 0.03, axis=1, bitorder="little"), rep, axis=0)
    nq = m * rep
    valid = np.ones(nq, np.int32); obs = np.ones(nq, np.int32)
    octave = np.full(nq, CROWD_OCTAVE, np.int32); angle = np.zeros(nq, np.float32)
    T = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(np.float32)  # no motion: levels octave - 1 .. octave + 1
    sf = O.Extractor().scale_factors()
    g = case["grid"]
    th = 7.0
    admissible = [int((has[g.features_in_area(float(a), float(b), float(np.float32(th) * sf[CROWD_OCTAVE]), CROWD_OCTAVE - 1, CROWD_OCTAVE + 1)] == 0).sum())
                  for a, b in zip(u, v)]
    if case["n"] >= 1023:
        assert min(admissible) > 256
    ref, nref = O.search_by_projection_last(g, ur, d, sf, CAM, T, T, pos, desc, valid, obs, octave, angle, has, th, True, False)
    got, ngot = ctx.search_by_projection_last(ctx._view(k, ur, d, BOUNDS), T, T, pos, desc, valid, obs, octave, angle, has, th, True, False)
    assert ngot == nref and np.array_equal(got, ref)
    assert nref == min(nq, int((has[case["crowd"]] == 0).sum()))  # every query took a free keypoint of the crowd until none was left
