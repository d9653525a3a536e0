"""HIP == oracle on the tails of Frame::ComputeStereoMatches (src/Frame.cc:596-641) and ComputeStereoFromRGBD (:645-666).

The inputs are those of tests/stereo_census.py, whose CPU census (tests/test_stereo_census.py) shows which branch each one
reaches: negative disparities, the 0.01 clamp, disparity >= maxD, a median of 0, no accepted match, bf == 0, deltaR == 0.5,
Hamming and SAD ties, tiny match counts.  uRight and depth are compared with array_equal, single frames and one batched call.
The RGB-D twin is fed the depth values a sensor map can hold besides positive numbers and exact-0 holes.
"""
import numpy as np
import pytest

from oracle import oracle as O
from orbslam2_amd import synth
from tests import stereo_census as S

pytestmark = pytest.mark.gpu


def _ctx(cfg, max_images=2):
    from orbslam2_amd import api
    return api.Context(max_images=max_images, **cfg)


def _oracle(name):
    cfg, left, right, branch = S.build(name)
    exl, exr, kl, dl, kr, dr = S.oracle_frame(cfg, left, right)
    ur, dp, m = O.stereo_matches(exl, exr, kl, dl, kr, dr, cfg["bf"], cfg["fx"])
    return dict(cfg=cfg, left=left, right=right, branch=branch, kl=kl, dl=dl, kr=kr, dr=dr, ur=ur, dp=dp, m=m)


def _assert_kps_equal(got, ref, what):
    assert len(got) == len(ref), "%s: %d vs %d keypoints" % (what, len(got), len(ref))
    for f in ("octave", "x", "y", "response", "size", "angle", "class_id"):
        bad = np.nonzero(got[f] != ref[f])[0]
        assert bad.size == 0, "%s: field %s differs at %s (got %s ref %s)" % (
            what, f, bad[:5].tolist(), got[f][bad[:5]].tolist(), ref[f][bad[:5]].tolist())


def _assert_stereo_equal(got_u, got_d, ur, dp, what):
    assert len(got_u) == len(ur), what
    assert np.array_equal(got_u < 0, ur < 0), "%s: matched sets differ at %s" % (what, np.nonzero((got_u < 0) != (ur < 0))[0][:8].tolist())
    bad = np.nonzero((got_u != ur) | (got_d != dp))[0]
    assert np.array_equal(got_u, ur), "%s: u_right not bit-exact: max diff %g, first at %s (got %s ref %s)" % (
        what, np.abs(got_u - ur).max(), bad[:5].tolist(), got_u[bad[:5]].tolist(), ur[bad[:5]].tolist())
    assert np.array_equal(got_d, dp), "%s: depth not bit-exact: max rel diff %g, first at %s (got %s ref %s)" % (
        what, np.abs((got_d - dp) / np.maximum(dp, 1e-9)).max(), bad[:5].tolist(), got_d[bad[:5]].tolist(), dp[bad[:5]].tolist())


@pytest.mark.parametrize("name", list(S.INPUTS))
def test_single_frame_equals_oracle(name):
    o = _oracle(name)
    what = "%s [built for: %s]" % (name, o["branch"])
    ctx = _ctx(o["cfg"])  # bf == 0 included: the context must be created
    out = ctx.stereo_frame(o["left"], o["right"])
    _assert_kps_equal(out["kps_left"], o["kl"], what + " left")
    _assert_kps_equal(out["kps_right"], o["kr"], what + " right")
    assert np.array_equal(out["desc_left"], o["dl"]) and np.array_equal(out["desc_right"], o["dr"]), what
    _assert_stereo_equal(out["u_right"], out["depth"], o["ur"], o["dp"], what)
    assert o["m"] == int((o["ur"] >= 0).sum())
    again = ctx.stereo_frame(o["left"], o["right"])  # the per-pair SAD tap and row lists of the first call are overwritten, not merged
    _assert_stereo_equal(again["u_right"], again["depth"], o["ur"], o["dp"], what + " second call")
    ctx.close()


def test_bf_zero_matches_nothing():
    """bf == 0: the reference returns before the search (mb == 0, :494); the kernel gets there through maxD = 0 / 0 = NaN,
    a bound no candidate passes.  Both routes leave every keypoint at -1."""
    o = _oracle("bf0")
    assert o["cfg"]["bf"] == 0.0 and len(o["kl"]) >= 500 and len(o["kr"]) >= 500
    ctx = _ctx(o["cfg"])
    out = ctx.stereo_frame(o["left"], o["right"])
    assert len(out["u_right"]) == len(o["kl"])
    assert (out["u_right"] == -1).all() and (out["depth"] == -1).all()
    assert (o["ur"] == -1).all() and (o["dp"] == -1).all()
    ctx.close()


@pytest.fixture(scope="module")
def batch():
    import torch
    from orbslam2_amd import api
    orc = [_oracle(name) for name in S.BATCH]
    assert all(o["cfg"] == S.BASE for o in orc)
    single = api.Context(max_images=2, **S.BASE)
    ref = [single.stereo_frame(o["left"], o["right"]) for o in orc]
    single.close()
    host = np.stack([im for o in orc for im in (o["left"], o["right"])])
    return dict(torch=torch, api=api, orc=orc, ref=ref, dev=torch.from_numpy(host).cuda())


@pytest.mark.parametrize("groups", [1, 2])
def test_one_batched_call_keeps_the_pairs_apart(batch, groups):
    """ordinary, identical (median 0: all cut), right image flat (no match: the median launch returns early), composite (clamp
    survives), ordinary -- in ONE orbfe_enqueue_stereo call: every pair equals its single-frame result and the oracle, so the
    median launch keeps its per-pair state apart."""
    api, torch = batch["api"], batch["torch"]
    n = len(S.BATCH)
    ctx = api.Context(max_images=2 * n, **S.BASE)
    ctx.set_streams(groups)
    for rep in range(2):  # second pass reuses every buffer
        ctx.enqueue_stereo(batch["dev"].data_ptr(), n, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        counts = ctx.fetch_counts(2 * n)
        for i, (name, o, ref) in enumerate(zip(S.BATCH, batch["orc"], batch["ref"])):
            what = "groups %d pass %d slot %d: %s [built for: %s]" % (groups, rep, i, name, o["branch"])
            left = ctx.fetch_image(2 * i, stereo=True)
            right = ctx.fetch_image(2 * i + 1)
            assert counts[2 * i] == len(o["kl"]) and counts[2 * i + 1] == len(o["kr"]), what
            _assert_kps_equal(left["kps"], o["kl"], what + " left")
            _assert_kps_equal(right["kps"], o["kr"], what + " right")
            assert np.array_equal(left["desc"], o["dl"]) and np.array_equal(right["desc"], o["dr"]), what
            _assert_stereo_equal(left["u_right"], left["depth"], ref["u_right"], ref["depth"], what + " vs single frame")
            _assert_stereo_equal(left["u_right"], left["depth"], o["ur"], o["dp"], what + " vs oracle")
    # the batch holds what it was built for
    m = [int((o["ur"] >= 0).sum()) for o in batch["orc"]]
    assert m[0] > 100 and m[1] == 0 and m[2] == 0 and m[3] > 100 and m[4] > 100
    assert len(batch["orc"][2]["kr"]) == 0 and len(batch["orc"][2]["kl"]) >= 500
    bf = np.float32(S.BASE["bf"])
    assert int((batch["orc"][3]["dp"] == bf / np.float32(0.01)).sum()) >= 10
    ctx.close()


@pytest.mark.parametrize("groups", [1, 2])
def test_packed_fetch_of_the_batch(batch, groups):
    """The same batch through ORBFE_PACK_STEREO: the expanded u_right / depth equal the unpacked ones."""
    api, torch = batch["api"], batch["torch"]
    n = len(S.BATCH)
    ctx = api.Context(max_images=2 * n, **S.BASE)
    ctx.set_streams(groups)
    ctx.enqueue_stereo(batch["dev"].data_ptr(), n, 0)
    for flags in (api.PACK_STEREO, api.PACK_STEREO | api.PACK_LEFT_ONLY):
        block, lay = ctx.fetch_packed(2 * n, flags)
        step = 2 if flags & api.PACK_LEFT_ONLY else 1
        for i, (name, o) in enumerate(zip(S.BATCH, batch["orc"])):
            what = "flags %d slot %d: %s [built for: %s]" % (flags, i, name, o["branch"])
            unpacked = ctx.fetch_image(2 * i, stereo=True)
            got = ctx.expand_packed(block, lay, 2 * i // step)
            assert got["kps"].tobytes() == unpacked["kps"].tobytes() and np.array_equal(got["desc"], unpacked["desc"]), what
            assert got["u_right"].tobytes() == unpacked["u_right"].tobytes() and got["depth"].tobytes() == unpacked["depth"].tobytes(), what
            _assert_stereo_equal(got["u_right"], got["depth"], o["ur"], o["dp"], what + " vs oracle")
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# RGB-D tail
# ---------------------------------------------------------------------------------------------------------------------
DENORM_MIN = np.float32(1.401298464324817e-45)
SPECIAL_F32 = [np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), np.float32(-1.0), np.float32(-0.0), DENORM_MIN,
               np.float32(1e-30), np.float32(1e30)]
SPECIAL_U16 = [0, 1, 65535]
TUM1_DIST = [0.262383, -0.953104, -0.005358, 0.002628, 1.163314]  # Examples/RGB-D/TUM1.yaml


def _plant(depth, k, values, rot=0):
    """Write values[j] under the keypoints whose pixel (int)kp.y, (int)kp.x is the (j + rot)-th, (j + rot + nv)-th, .. distinct
    one of every third; returns the number of keypoints that read each value."""
    out = depth.copy()
    px = np.stack([k["y"].astype(np.int64), k["x"].astype(np.int64)], 1)
    uniq = np.unique(px, axis=0)[::3]
    nv = len(values)
    for j, v in enumerate(values):
        sel = uniq[(j + rot) % nv::nv]
        out[sel[:, 0], sel[:, 1]] = v
    seen = out[px[:, 0], px[:, 1]]
    counts = [int(np.isnan(seen).sum()) if v != v else int(((seen == v) & (np.signbit(seen) == np.signbit(v))).sum()) for v in values]
    return out, counts


def _rgbd_oracle(cfg, k, depth_f32, dist=None):
    kun = k
    if dist is not None:
        und = O.undistort_points(np.stack([k["x"], k["y"]], 1), cfg["fx"], cfg["fy"], cfg["cx"], cfg["cy"], dist)
        kun = k.copy(); kun["x"], kun["y"] = und[:, 0], und[:, 1]
    return O.stereo_from_rgbd(k, kun, depth_f32, cfg["bf"])


def _expect_f32(k_x, seen, ur, dp, bf):
    """What the reference writes (:658-664), spelled out per planted value, NaN-free by construction."""
    neg = ~(seen > 0)  # NaN, -inf, -1, -0.0, 0 holes
    assert (ur[neg] == -1).all() and (dp[neg] == -1).all()
    assert not np.isnan(ur).any() and not np.isnan(dp).any()
    inf = np.isposinf(seen)
    assert np.isposinf(dp[inf]).all() and np.array_equal(ur[inf], k_x[inf])  # x - bf / inf = x - 0
    den = seen == DENORM_MIN
    assert (dp[den] == DENORM_MIN).all() and np.isneginf(ur[den]).all()  # bf / denormal overflows: x - inf
    tiny = seen == np.float32(1e-30)
    assert np.array_equal(ur[tiny], k_x[tiny] - np.float32(bf) / np.float32(1e-30)) and (ur[tiny] < -1e30).all()
    huge = seen == np.float32(1e30)
    assert (dp[huge] == np.float32(1e30)).all() and np.array_equal(ur[huge], k_x[huge])


@pytest.mark.parametrize("dist", [None, TUM1_DIST], ids=["undistorted", "tum1-distortion"])
def test_rgbd_special_depth_values(dist):
    """NaN, +-inf, -1, -0.0, the smallest denormal, 1e-30 and 1e30 under >= 20 keypoints each: rgbd_frame == the oracle, which
    writes -1 for !(d > 0), depth = inf / uRight = x for +inf, and uRight = -inf for a denormal depth.  With distortion set,
    uRight comes from the undistorted x while the depth is read at the distorted pixel."""
    import torch
    cfg = S.BASE
    frames = []
    for i in range(3):
        gray, _, depth = synth.stereo_pair(cfg["width"], cfg["height"], seed=40 + i, with_depth=True, bf=cfg["bf"])
        k, d = O.Extractor(**S.extractor_kwargs(cfg)).extract(gray)
        planted, counts = _plant(depth, k, SPECIAL_F32, rot=i)
        assert min(counts) >= 20, counts
        ur, dp = _rgbd_oracle(cfg, k, planted, dist)
        seen = planted[k["y"].astype(np.int64), k["x"].astype(np.int64)]
        if dist is None:
            _expect_f32(k["x"], seen, ur, dp, cfg["bf"])
        assert (dp > 0).sum() > 300 and (seen == 0).sum() > 0  # ordinary depths and the synthetic map's exact-0 holes as well
        frames.append(dict(gray=gray, depth=planted, k=k, d=d, ur=ur, dp=dp))
    ctx = _ctx(cfg, max_images=3)
    if dist is not None:
        ctx.set_distortion(dist)
    for i, f in enumerate(frames):
        out = ctx.rgbd_frame(f["gray"], f["depth"])
        _assert_kps_equal(out["kps"], f["k"], "rgbd frame %d" % i)
        assert np.array_equal(out["desc"], f["d"])
        _assert_stereo_equal(out["u_right"], out["depth"], f["ur"], f["dp"], "rgbd_frame %d" % i)
    if dist is not None:
        ur0, _ = _rgbd_oracle(cfg, frames[0]["k"], frames[0]["depth"])
        assert not np.array_equal(ur0, frames[0]["ur"])
    d_gray = torch.from_numpy(np.stack([f["gray"] for f in frames])).cuda()
    d_depth = torch.from_numpy(np.stack([f["depth"] for f in frames])).cuda()
    ctx.enqueue_rgbd(d_gray.data_ptr(), d_depth.data_ptr(), 3)
    ctx.synchronize()
    for i, f in enumerate(frames):
        got = ctx.fetch_image(i, stereo=True)
        _assert_kps_equal(got["kps"], f["k"], "enqueue_rgbd frame %d" % i)
        _assert_stereo_equal(got["u_right"], got["depth"], f["ur"], f["dp"], "enqueue_rgbd frame %d" % i)
    ctx.close()


@pytest.mark.parametrize("dist", [None, TUM1_DIST], ids=["undistorted", "tum1-distortion"])
def test_rgbd_raw_u16_extremes(dist):
    """A raw sensor map holding 0, 1 and 65535 under >= 20 keypoints each, depth_map_factor = 1 / 5000 (TUM)."""
    import torch
    cfg = S.BASE
    factor = np.float32(1.0) / np.float32(5000.0)
    frames = []
    for i in range(3):
        gray, _, depth = synth.stereo_pair(cfg["width"], cfg["height"], seed=50 + i, with_depth=True, bf=40.0)  # depths below 13.1 m: inside the u16 range
        raw = np.clip(np.rint(depth * 5000.0), 0, 65535).astype(np.uint16)
        k, d = O.Extractor(**S.extractor_kwargs(cfg)).extract(gray)
        px = np.unique(np.stack([k["y"].astype(np.int64), k["x"].astype(np.int64)], 1), axis=0)[::3]
        for j, v in enumerate(SPECIAL_U16):
            sel = px[(j + i) % 3::3]
            raw[sel[:, 0], sel[:, 1]] = v
        seen = raw[k["y"].astype(np.int64), k["x"].astype(np.int64)]
        assert min(int((seen == v).sum()) for v in SPECIAL_U16) >= 20
        conv = raw.astype(np.float32) * factor  # convertTo(CV_32F, mDepthMapFactor): one rounded float multiply
        ur, dp = _rgbd_oracle(cfg, k, conv, dist)
        assert (dp[seen == 0] == -1).all() and (dp[seen == 1] == factor).all() and (dp[seen == 65535] == np.float32(65535) * factor).all()
        frames.append(dict(gray=gray, raw=raw, k=k, d=d, ur=ur, dp=dp))
    ctx = _ctx(cfg, max_images=3)
    if dist is not None:
        ctx.set_distortion(dist)
    for i, f in enumerate(frames):
        out = ctx.rgbd_frame(f["gray"], f["raw"], depth_map_factor=float(factor))
        _assert_kps_equal(out["kps"], f["k"], "rgbd u16 frame %d" % i)
        _assert_stereo_equal(out["u_right"], out["depth"], f["ur"], f["dp"], "rgbd_frame u16 %d" % i)
    d_gray = torch.from_numpy(np.stack([f["gray"] for f in frames])).cuda()
    d_depth = torch.from_numpy(np.stack([f["raw"] for f in frames]).view(np.int16)).cuda()  # torch has no uint16 on every build: same bytes
    ctx.enqueue_rgbd(d_gray.data_ptr(), d_depth.data_ptr(), 3, depth_is_u16=True, depth_map_factor=float(factor))
    ctx.synchronize()
    for i, f in enumerate(frames):
        got = ctx.fetch_image(i, stereo=True)
        _assert_stereo_equal(got["u_right"], got["depth"], f["ur"], f["dp"], "enqueue_rgbd u16 frame %d" % i)
    ctx.close()
