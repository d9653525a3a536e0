"""The per-frame matchers of Tracking on device-resident data (orbfe_enqueue_search_by_projection_last, orbfe_enqueue_is_in_frustum,
orbfe_enqueue_search_by_projection_points, orbfe_device_keys_un; orbslam2_amd/csrc/orbfe_match_device.hip): device pointers in,
matches in HBM, asynchronous on a caller-owned stream.  Every comparison is exact, against the CPU oracle AND against the
synchronous entry point on the same inputs (projection on the host, greedy accept rules replayed on the host).

Device memory is torch tensors.  A synthetic frame (keypoint-level scenes of tests/test_matchers.py) becomes "image slot 0 of
the latest extraction call" by one real extraction call of the same context -- which fixes the call the slot belongs to --
followed by torch copies of the keypoints, descriptors, uRight and the count into the context's device buffers
(orbfe_device_buffers); tests that say "real frame" match against what the extraction itself left there.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import test_matchers as TM
from tests.device_arrays import UNTOUCHED, context, device_buffers, raw, upload

W, H, FX, FY, CX, CY, BF, NL = TM.W, TM.H, TM.FX, TM.FY, TM.CX, TM.CY, TM.BF, TM.NL
NEW = ["orbfe_enqueue_search_by_projection_last", "orbfe_enqueue_is_in_frustum", "orbfe_enqueue_search_by_projection_points",
       "orbfe_device_keys_un"]


# ------------------------------------------------------------------ CPU
def test_the_library_exports_the_enqueue_matchers_and_they_refuse_a_null_context():
    from orbslam2_amd import api
    L = api.load()
    for name in NEW:
        assert name in api.EXPORTS
        fn = getattr(L, name)  # AttributeError: the symbol is not exported
        args = [0 if t is C.c_int else 0.0 if t is C.c_float else None for t in fn.argtypes]
        assert fn(*args) == api.ERR_INVALID, name
    for m in ("enqueue_search_by_projection_last", "enqueue_is_in_frustum", "enqueue_search_by_projection_points", "device_keys_un"):
        assert callable(getattr(api.Context, m))


# ------------------------------------------------------------------ helpers (GPU)
def _inject(ctx, k, d, ur, seed=501):
    """Makes (k, d, ur) image slot 0 of a fresh extraction call of `ctx` (see the module docstring)."""
    import torch
    from orbslam2_amd import synth
    left, right = synth.stereo_pair(W, H, seed=seed)
    ctx.stereo_frame(left, right)
    n = len(k)
    assert n <= ctx.capacity
    b = device_buffers(ctx)
    raw(b["kps"], 28 * ctx.capacity)[: 28 * n] = upload(np.ascontiguousarray(k, O.KP_DTYPE))[0]
    raw(b["desc"], 32 * ctx.capacity)[: 32 * n] = upload(np.ascontiguousarray(d, np.uint8).reshape(-1))[0]
    raw(b["u_right"], 4 * ctx.capacity)[: 4 * n] = upload(np.ascontiguousarray(ur, np.float32).view(np.uint8))[0]
    raw(b["counts"], 4)[:] = upload(np.array([n], np.int32).view(np.uint8))[0]
    torch.cuda.synchronize()


class _Out:
    def __init__(self, cap, pose=False):
        import torch
        self.match = torch.full((cap,), UNTOUCHED, dtype=torch.int32, device="cuda:0")
        self.nm = torch.full((1,), UNTOUCHED, dtype=torch.int32, device="cuda:0")
        self.status = torch.full((1,), UNTOUCHED, dtype=torch.int32, device="cuda:0")
        self.has = torch.zeros(cap, dtype=torch.uint8, device="cuda:0") if pose else None
        self.Xw = torch.zeros((cap, 3), dtype=torch.float32, device="cuda:0") if pose else None

    def check(self, ref, nref, what=""):
        """After the stream was synchronised: exactly the reference, nothing written past the frame's keypoints."""
        got = self.match.cpu().numpy()
        n = len(ref)
        assert int(self.status.item()) == 0, what
        assert int(self.nm.item()) == nref, (what, int(self.nm.item()), nref)
        assert np.array_equal(got[:n], ref), what
        assert (got[n:] == UNTOUCHED).all(), what


class _Last:
    """The last frame's arrays in HBM, uploaded once."""

    def __init__(self, T_cur, T_last, pos, desc, valid, obs, octave, angle, has):
        self.n = len(valid)
        self.keep = [upload(np.ascontiguousarray(x, t))[0] for x, t in ((T_cur, np.float32), (T_last, np.float32), (pos, np.float32), (desc, np.uint8),
                                                                   (valid, np.int32), (obs, np.int32), (octave, np.int32), (angle, np.float32))]
        self.has = None if has is None else upload(np.ascontiguousarray(has, np.uint8))[0]

    def enqueue(self, ctx, slot, bounds, th, mono, ori, out, stream):
        p = [t.data_ptr() if t.numel() else 0 for t in self.keep]
        ctx.enqueue_search_by_projection_last(slot, bounds, p[0], p[1], self.n, p[2], p[3], p[4], p[5], p[6], p[7],
                                              0 if self.has is None else self.has.data_ptr(), th, mono, ori, out.match.data_ptr(),
                                              out.nm.data_ptr(), out.status.data_ptr(), 0 if out.has is None else out.has.data_ptr(),
                                              0 if out.Xw is None else out.Xw.data_ptr(), stream.cuda_stream)


def _last_of(s, has_key="has", desc_key="desc"):
    return _Last(s["T_cur"], s["T_last"], s["pos"], s[desc_key], s["valid"], s["obs"], s["octave"], s["angle"], s[has_key])


def _prefix_scene():
    """The scene of test_gpu_topk_prefix_runs_out_and_the_full_list_takes_over (tests/test_matchers.py): 60 clusters of 8 near-copies
    of a map point's keypoint, every map point 10 times -- copies 5 .. 8 find all four keys of their prefix taken."""
    s = TM._scene(90, n_last=150, n_distract=700)
    rng = np.random.default_rng(91)
    T = s["T_cur"].astype(np.float64)
    pc = (T[:, :3] @ s["pos"].T.astype(np.float64)).T + T[:, 3]
    uu = FX * pc[:, 0] / pc[:, 2] + CX; vv = FY * pc[:, 1] / pc[:, 2] + CY
    ok = np.nonzero((s["valid"] == 1) & (pc[:, 2] > 0.5) & (uu > 30) & (uu < W - 30) & (vv > 30) & (vv < H - 30))[0][:60]
    extra_k = np.zeros(len(ok) * 8, O.KP_DTYPE); extra_d = np.zeros((len(ok) * 8, 32), np.uint8)
    for a_, i in enumerate(ok):
        for j in range(8):
            e = a_ * 8 + j
            extra_k["x"][e] = uu[i] + rng.uniform(-1, 1); extra_k["y"][e] = vv[i] + rng.uniform(-1, 1)
            extra_k["octave"][e] = s["octave"][i]; extra_k["angle"][e] = s["angle"][i]
            bits = np.zeros(256, bool); bits[rng.permutation(256)[:j]] = True  # j bits away from the map point's descriptor
            extra_d[e] = s["desc_last"][i] ^ np.packbits(bits, bitorder="little")
    extra_k["size"] = 31; extra_k["class_id"] = -1
    k = np.concatenate([s["k"], extra_k]); d = np.concatenate([s["d"], extra_d])
    ur = np.concatenate([s["ur"], np.full(len(extra_k), -1.0, np.float32)])
    has = np.concatenate([s["cur_has_obs"], np.zeros(len(extra_k), np.uint8)])
    rep = 10
    out = dict(k=k, d=d, ur=ur, has=has, bounds=s["bounds"], sf=s["sf"], T_cur=s["T_cur"], T_last=s["T_last"], n_clusters=len(ok),
               pos=np.repeat(s["pos"], rep, axis=0), desc=np.repeat(s["desc_last"], rep, axis=0), valid=np.repeat(s["valid"], rep),
               octave=np.repeat(s["octave"], rep), angle=np.repeat(s["angle"], rep), rng=rng)
    tp = np.zeros(len(out["pos"]), O.TP_DTYPE)
    tp["in_view"] = out["valid"]; tp["proj_x"] = np.repeat(uu, rep); tp["proj_y"] = np.repeat(vv, rep); tp["proj_xr"] = -1
    tp["level"] = out["octave"]; tp["view_cos"] = 0.9
    tp["in_view"][(tp["proj_x"] < 0) | (tp["proj_x"] > W) | (tp["proj_y"] < 0) | (tp["proj_y"] > H)] = 0
    out["tp"] = tp
    return out


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("distorted", [False, True])
def test_gpu_enqueue_last_on_a_real_extracted_frame(distorted):
    """Real frames (synth.stereo_pair through stereo_frame, slot 0), two successive frames of one context; on each frame:
    asynchronous call, synchronous resident call, asynchronous call again -- all equal to the oracle."""
    import torch
    from orbslam2_amd import api, synth
    ctx = context(api, nfeatures=1500)
    dist = [-0.28, 0.07, 2e-4, 1e-5, 0.0]
    if distorted:
        ctx.set_distortion(dist)
    st = torch.cuda.Stream()
    sf = O.Extractor().scale_factors()
    for rep, seed in enumerate((501, 502)):
        left, right = synth.stereo_pair(W, H, seed=seed)
        fr = ctx.stereo_frame(left, right)
        k, d, ur = fr["kps_left"], fr["desc_left"], fr["u_right"]
        kun = ctx.fetch_keys_un(0) if distorted else k
        bounds = tuple(float(b) for b in ctx.image_bounds()) if distorted else (0.0, float(W), 0.0, float(H))
        s = TM._frame_scene(kun, d, ur, seed)
        last = _last_of(s)
        g = O.Grid(kun, *bounds)
        for th, mono, ori in ((7.0, False, True), (15.0, True, False)):
            u = None if mono else ur
            ref, nref = O.search_by_projection_last(g, u, d, sf, TM.CAM, s["T_cur"], s["T_last"], s["pos"], s["desc"], s["valid"], s["obs"],
                                                    s["octave"], s["angle"], s["has"], th, mono, ori)
            assert nref > 40
            vd = ctx._view(kun, u, d, bounds, device_slot=0)
            for step in ("async", "sync", "async"):
                if step == "sync":
                    got, ngot = ctx.search_by_projection_last(vd, s["T_cur"], s["T_last"], s["pos"], s["desc"], s["valid"], s["obs"], s["octave"],
                                                              s["angle"], s["has"], th, mono, ori)
                    assert ngot == nref and np.array_equal(got, ref), (rep, th)
                    continue
                out = _Out(ctx.capacity)
                torch.cuda.synchronize()
                last.enqueue(ctx, 0, bounds, th, mono, ori, out, st)
                st.synchronize()
                out.check(ref, nref, (rep, th, step))
    # host-visible argument errors: refused at once
    out = _Out(ctx.capacity)
    with pytest.raises(api.OrbfeError):
        last.enqueue(ctx, 5, bounds, 7.0, False, True, out, st)  # no such slot
    with pytest.raises(api.OrbfeError):
        ctx.enqueue_search_by_projection_last(0, bounds, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 7.0, False, True, out.match.data_ptr(), out.nm.data_ptr(),
                                              out.status.data_ptr(), stream=st.cuda_stream)  # no poses
    ctx.close()


@pytest.mark.gpu
def test_gpu_enqueue_last_batched_back_to_back():
    """enqueue_stereo of 4 pairs, then the matcher on slots 0, 2, 4, 6 queued back to back on the same stream with no
    synchronisation in between; one synchronise at the end.  Real frames."""
    import torch
    from orbslam2_amd import api, synth
    ctx = context(api, nfeatures=1200, max_images=8)
    imgs = []
    for seed in (601, 602, 603, 604):
        left, right = synth.stereo_pair(W, H, seed=seed)
        imgs += [left, right]
    d_img = upload(np.stack(imgs).astype(np.uint8))[0]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    ctx.enqueue_stereo(d_img.data_ptr(), 4, st.cuda_stream)
    ctx.synchronize(st.cuda_stream)
    bounds = (0.0, float(W), 0.0, float(H))
    sf = O.Extractor().scale_factors()
    cases = []
    for p in range(4):
        fr = ctx.fetch_image(2 * p, stereo=True)
        k, d, ur = fr["kps"], fr["desc"], fr["u_right"]
        s = TM._frame_scene(k, d, ur, 610 + p)
        ref, nref = O.search_by_projection_last(O.Grid(k, *bounds), ur, d, sf, TM.CAM, s["T_cur"], s["T_last"], s["pos"], s["desc"], s["valid"],
                                                s["obs"], s["octave"], s["angle"], s["has"], 7.0, False, True)
        assert nref > 40
        cases.append((_last_of(s), _Out(ctx.capacity), ref, nref))
    torch.cuda.synchronize()
    ctx.enqueue_stereo(d_img.data_ptr(), 4, st.cuda_stream)  # the same frames again: a new extraction call, nothing fetched in between
    for p, (last, out, _, _) in enumerate(cases):
        last.enqueue(ctx, 2 * p, bounds, 7.0, False, True, out, st)
    st.synchronize()
    for p, (_, out, ref, nref) in enumerate(cases):
        out.check(ref, nref, p)
    ctx.close()


# camera moved forward by more than bf / fx = 0.1, backward by more, and sideways (neither): the three level windows
MOTIONS = {"forward": (2.0, [0.02, -0.01, -0.3]), "backward": (-1.0, [0.0, 0.0, 0.4]), "neither": (1.0, [0.25, 0.0, 0.03])}


@pytest.mark.gpu
@pytest.mark.parametrize("motion", sorted(MOTIONS))
def test_gpu_enqueue_last_forward_backward_neither(motion):
    """Synthetic current frame (TM._scene seed 12) put into slot 0, see the module docstring."""
    import torch
    from orbslam2_amd import api
    s = TM._scene(12)
    s["T_cur"] = TM._se3(*MOTIONS[motion])
    twc = -s["T_cur"][:, :3].T.astype(np.float64) @ s["T_cur"][:, 3].astype(np.float64)
    assert {"forward": twc[2] > BF / FX, "backward": -twc[2] > BF / FX, "neither": abs(twc[2]) < BF / FX}[motion]  # T_last = identity
    ref, nref = O.search_by_projection_last(O.Grid(s["k"], *s["bounds"]), s["ur"], s["d"], s["sf"], TM.CAM, s["T_cur"], s["T_last"], s["pos"],
                                            s["desc_last"], s["valid"], s["obs"], s["octave"], s["angle"], s["cur_has_obs"], 14.0, False, False)
    assert nref > 50
    ctx = context(api)
    got, ngot = ctx.search_by_projection_last(ctx._view(s["k"], s["ur"], s["d"], s["bounds"]), s["T_cur"], s["T_last"], s["pos"], s["desc_last"],
                                              s["valid"], s["obs"], s["octave"], s["angle"], s["cur_has_obs"], 14.0, False, False)
    assert ngot == nref and np.array_equal(got, ref)
    _inject(ctx, s["k"], s["d"], s["ur"])
    out = _Out(ctx.capacity)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    _last_of(s, "cur_has_obs", "desc_last").enqueue(ctx, 0, s["bounds"], 14.0, False, False, out, st)
    st.synchronize()
    out.check(ref, nref, motion)
    ctx.close()


@pytest.mark.gpu
def test_gpu_enqueue_prefix_runs_out_and_the_window_is_scanned_again():
    """Synthetic frame in slot 0.  With Observations() > 0 everywhere the clusters are used up and copies 5 .. 8 need keys beyond
    their four-key prefix; with Observations() == 0 everywhere nothing is ever blocked, every copy takes the same keypoint and
    the reference's counter counts each (the double-count rule); then a mix with the rotation check on."""
    import torch
    from orbslam2_amd import api
    p = _prefix_scene()
    g = O.Grid(p["k"], *p["bounds"])
    ctx = context(api)
    view = ctx._view(p["k"], p["ur"], p["d"], p["bounds"])
    _inject(ctx, p["k"], p["d"], p["ur"])
    st = torch.cuda.Stream()
    n = len(p["pos"])

    def last(obs, angle, th, ori, what):
        ref, nref = O.search_by_projection_last(g, p["ur"], p["d"], p["sf"], TM.CAM, p["T_cur"], p["T_last"], p["pos"], p["desc"], p["valid"], obs,
                                                p["octave"], angle, p["has"], th, False, ori)
        got, ngot = ctx.search_by_projection_last(view, p["T_cur"], p["T_last"], p["pos"], p["desc"], p["valid"], obs, p["octave"], angle,
                                                  p["has"], th, False, ori)
        assert ngot == nref and np.array_equal(got, ref), what
        out = _Out(ctx.capacity)
        torch.cuda.synchronize()
        _Last(p["T_cur"], p["T_last"], p["pos"], p["desc"], p["valid"], obs, p["octave"], angle, p["has"]).enqueue(ctx, 0, p["bounds"], th, False, ori, out, st)
        st.synchronize()
        out.check(ref, nref, what)
        return ref, nref

    ones, zeros = np.ones(n, np.int32), np.zeros(n, np.int32)
    for th, expect in ((7.0, 554), (120.0, 558)):
        ref, nref = last(ones, p["angle"], th, False, ("obs 1", th))
        assert nref == expect and nref == int((ref >= 0).sum()) and nref > 8 * p["n_clusters"] - 20
        ref, nref = last(zeros, p["angle"], th, False, ("obs 0", th))
        assert nref == 1000 and int((ref >= 0).sum()) == 100  # every copy counted, one keypoint per map point
    rng = np.random.default_rng(92)
    mixed = rng.integers(0, 2, n).astype(np.int32)
    angle = np.where(rng.random(n) < 0.3, rng.uniform(0, 360, n), p["angle"]).astype(np.float32)
    for th in (7.0, 120.0):
        _, n_off = last(mixed, angle, th, False, ("mixed, no rotation check", th))
        _, n_on = last(mixed, angle, th, True, ("mixed, rotation check", th))
        assert n_on < n_off  # the rotation check removed at least one match
    # SearchByProjection(F, points): best AND second best beyond the prefix
    d_tp, d_desc = upload(p["tp"])[0], upload(p["desc"])[0]
    d_has = upload(p["has"])[0]
    for obs, what in ((ones, "obs 1"), (zeros, "obs 0"), (mixed, "mixed")):
        ref, nref = O.search_by_projection_points(g, p["ur"], p["d"], p["sf"], p["tp"], p["desc"], obs, p["has"], 3.0, 0.99)
        got, ngot = ctx.search_by_projection_points(view, p["tp"], p["desc"], obs, p["has"], 3.0, 0.99)
        assert ngot == nref and np.array_equal(got, ref) and nref > 200, what
        out = _Out(ctx.capacity)
        d_obs = upload(obs)[0]
        torch.cuda.synchronize()
        ctx.enqueue_search_by_projection_points(0, p["bounds"], n, d_tp.data_ptr(), d_desc.data_ptr(), d_obs.data_ptr(), 0, d_has.data_ptr(), 3.0, 0.99,
                                                out.match.data_ptr(), out.nm.data_ptr(), out.status.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        out.check(ref, nref, what)
    ctx.close()


@pytest.mark.gpu
def test_gpu_enqueue_frustum_and_points():
    """Scene of test_gpu_frustum_and_search_by_projection_points (synthetic frame in slot 0): isInFrustum on the device, then
    SearchByProjection(F, points) fed by the device's own records."""
    import torch
    from orbslam2_amd import api
    s = TM._scene(20, n_last=1500)
    rng = s["rng"]
    n = len(s["pos"])
    normal = s["pos"] / np.linalg.norm(s["pos"], axis=1, keepdims=True) + rng.normal(0, 0.35, (n, 3))
    normal = (normal / np.linalg.norm(normal, axis=1, keepdims=True)).astype(np.float32)
    dist0 = np.linalg.norm(s["pos"], axis=1).astype(np.float32)
    max_d = (dist0 * rng.uniform(0.9, 3.0, n)).astype(np.float32); min_d = (max_d / np.float32(1.2 ** 7)).astype(np.float32)
    ref_tp = O.is_in_frustum(s["T_cur"], TM.CAM, s["bounds"], s["pos"], normal, max_d, min_d, 0.5, TM.LOG_SF, NL)
    assert ref_tp["in_view"].sum() > 300
    ctx = context(api)
    _inject(ctx, s["k"], s["d"], s["ur"])
    st = torch.cuda.Stream()
    d_T, d_pos, d_nr, d_mx, d_mn = upload(s["T_cur"])[0], upload(s["pos"])[0], upload(normal)[0], upload(max_d)[0], upload(min_d)[0]
    d_tp = torch.zeros(n * 24, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.enqueue_is_in_frustum(d_T.data_ptr(), s["bounds"], n, d_pos.data_ptr(), d_nr.data_ptr(), d_mx.data_ptr(), d_mn.data_ptr(), 0.5,
                              d_tp.data_ptr(), st.cuda_stream)
    st.synchronize()
    got_tp = d_tp.cpu().numpy().view(O.TP_DTYPE)
    assert np.array_equal(got_tp["in_view"], ref_tp["in_view"])
    v = ref_tp["in_view"] == 1
    for f in ("proj_x", "proj_y", "proj_xr", "level", "view_cos"):
        assert np.array_equal(got_tp[f][v], ref_tp[f][v]), f
    assert np.array_equal(got_tp, ctx.is_in_frustum(s["T_cur"], s["bounds"], s["pos"], normal, max_d, min_d, 0.5))  # the host entry point, all rows
    g = O.Grid(s["k"], *s["bounds"])
    view = ctx._view(s["k"], s["ur"], s["d"], s["bounds"])
    d_desc, d_obs, d_has = upload(s["desc_last"])[0], upload(s["obs"])[0], upload(s["cur_has_obs"])[0]
    for th, ratio in ((1.0, 0.8), (3.0, 0.8), (5.0, 0.6)):
        ref, nref = O.search_by_projection_points(g, s["ur"], s["d"], s["sf"], ref_tp, s["desc_last"], s["obs"], s["cur_has_obs"], th, ratio)
        assert nref > 100
        got, ngot = ctx.search_by_projection_points(view, ref_tp, s["desc_last"], s["obs"], s["cur_has_obs"], th, ratio)
        assert ngot == nref and np.array_equal(got, ref)
        out = _Out(ctx.capacity, pose=True)
        torch.cuda.synchronize()
        ctx.enqueue_is_in_frustum(d_T.data_ptr(), s["bounds"], n, d_pos.data_ptr(), d_nr.data_ptr(), d_mx.data_ptr(), d_mn.data_ptr(), 0.5,
                                  d_tp.data_ptr(), st.cuda_stream)
        ctx.enqueue_search_by_projection_points(0, s["bounds"], n, d_tp.data_ptr(), d_desc.data_ptr(), d_obs.data_ptr(), d_pos.data_ptr(),
                                                d_has.data_ptr(), th, ratio, out.match.data_ptr(), out.nm.data_ptr(), out.status.data_ptr(),
                                                out.has.data_ptr(), out.Xw.data_ptr(), st.cuda_stream)
        st.synchronize()
        out.check(ref, nref, th)
        has = out.has.cpu().numpy()[: len(ref)]
        assert np.array_equal(has, (ref >= 0).astype(np.uint8))
        assert np.array_equal(out.Xw.cpu().numpy()[: len(ref)][ref >= 0], s["pos"][ref[ref >= 0]])
    ctx.close()


@pytest.mark.gpu
def test_gpu_enqueue_edge_cases():
    """No map points; no valid map point; a frame without keypoints (flat image, real extraction); an octave out of range in a
    valid row is reported in d_status while the host call itself succeeds."""
    import torch
    from orbslam2_amd import api
    ctx = context(api)
    s = TM._scene(12)
    st = torch.cuda.Stream()
    _inject(ctx, s["k"], s["d"], s["ur"])
    nk = len(s["k"])
    none = np.full(nk, -1, np.int32)
    out = _Out(ctx.capacity)
    torch.cuda.synchronize()
    empty = _Last(s["T_cur"], s["T_last"], s["pos"][:0], s["desc_last"][:0], s["valid"][:0], s["obs"][:0], s["octave"][:0], s["angle"][:0], None)
    empty.enqueue(ctx, 0, s["bounds"], 7.0, False, True, out, st)
    st.synchronize()
    out.check(none, 0, "n_last == 0")
    out = _Out(ctx.capacity)
    torch.cuda.synchronize()
    _Last(s["T_cur"], s["T_last"], s["pos"], s["desc_last"], np.zeros_like(s["valid"]), s["obs"], s["octave"], s["angle"], s["cur_has_obs"]).enqueue(
        ctx, 0, s["bounds"], 7.0, False, True, out, st)
    st.synchronize()
    out.check(none, 0, "no valid row")
    octave = s["octave"].copy()
    octave[int(np.nonzero(s["valid"])[0][5])] = 99
    out = _Out(ctx.capacity)
    torch.cuda.synchronize()
    _Last(s["T_cur"], s["T_last"], s["pos"], s["desc_last"], s["valid"], s["obs"], octave, s["angle"], s["cur_has_obs"]).enqueue(
        ctx, 0, s["bounds"], 7.0, False, True, out, st)  # returns ORBFE_OK (enqueue raises otherwise)
    st.synchronize()
    assert int(out.status.item()) == api.ERR_INVALID
    with pytest.raises(api.OrbfeError):  # the synchronous form sees the same row on the host
        ctx.search_by_projection_last(ctx._view(s["k"], s["ur"], s["d"], s["bounds"]), s["T_cur"], s["T_last"], s["pos"], s["desc_last"], s["valid"],
                                      s["obs"], octave, s["angle"], s["cur_has_obs"], 7.0, False, True)
    flat = np.full((H, W), 128, np.uint8)
    fr = ctx.stereo_frame(flat, flat)
    assert len(fr["kps_left"]) == 0
    out = _Out(ctx.capacity)
    torch.cuda.synchronize()
    last = _Last(s["T_cur"], s["T_last"], s["pos"], s["desc_last"], s["valid"], s["obs"], s["octave"], s["angle"], None)
    last.enqueue(ctx, 0, s["bounds"], 7.0, False, True, out, st)
    st.synchronize()
    out.check(np.zeros(0, np.int32), 0, "no keypoints")
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("distorted", [False, True])
def test_gpu_extraction_match_pose_on_one_stream(distorted):
    """enqueue_stereo -> enqueue_search_by_projection_last (has_point / Xw) -> orbfe_device_keys_un ->
    orbfe_enqueue_pose_optimization on one stream with one synchronise.  Matches equal the oracle's; pose, outlier flags and
    inlier count are bit-equal to the host entry point fed with the same keys, uRight, has_point and Xw (same kernel)."""
    import torch
    from orbslam2_amd import api, synth
    ctx = context(api, nfeatures=1500)
    if distorted:
        ctx.set_distortion([-0.28, 0.07, 2e-4, 1e-5, 0.0])
    left, right = synth.stereo_pair(W, H, seed=701)
    d_img = upload(np.stack([left, right]).astype(np.uint8))[0]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    ctx.enqueue_stereo(d_img.data_ptr(), 1, st.cuda_stream)
    ctx.synchronize(st.cuda_stream)
    fr = ctx.fetch_image(0, stereo=True)
    k, d, ur = fr["kps"], fr["desc"], fr["u_right"]
    kun = ctx.fetch_keys_un(0) if distorted else k
    bounds = tuple(float(b) for b in ctx.image_bounds()) if distorted else (0.0, float(W), 0.0, float(H))
    s = TM._frame_scene(kun, d, ur, 701)
    sf = O.Extractor().scale_factors()
    ref, nref = O.search_by_projection_last(O.Grid(kun, *bounds), ur, d, sf, TM.CAM, s["T_cur"], s["T_last"], s["pos"], s["desc"], s["valid"],
                                            s["obs"], s["octave"], s["angle"], s["has"], 7.0, False, True)
    assert nref > 40
    T0 = np.eye(4, dtype=np.float32); T0[:3] = s["T_cur"]
    has_point = (ref >= 0).astype(np.uint8)
    Xw = np.zeros((len(kun), 3), np.float32); Xw[ref >= 0] = s["pos"][ref[ref >= 0]]
    T_host, out_host, n_host = ctx.pose_optimization(T0, kun, ur, has_point, Xw)
    assert n_host > 20
    # the chain; nothing is fetched and nothing waits until the end
    b = device_buffers(ctx)
    last = _last_of(s)
    out = _Out(ctx.capacity, pose=True)
    d_T = upload(T0)[0]
    d_off = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    d_outlier = torch.zeros(ctx.capacity, dtype=torch.uint8, device="cuda:0")
    d_ninl = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    counts = raw(b["counts"], 4).view(torch.int32)
    torch.cuda.synchronize()
    ctx.enqueue_stereo(d_img.data_ptr(), 1, st.cuda_stream)
    last.keep[0] = d_T  # the 4x4 pose the optimisation will update: the matcher reads its first 12 floats
    last.enqueue(ctx, 0, bounds, 7.0, False, True, out, st)
    d_keys = ctx.device_keys_un(0, st.cuda_stream)
    with torch.cuda.stream(st):
        d_off[1:2] = counts  # offsets = [0, the slot's keypoint count], on the device
    ctx._check(ctx.L.orbfe_enqueue_pose_optimization(ctx.h, 1, d_off.data_ptr(), d_keys, b["u_right"], out.has.data_ptr(), out.Xw.data_ptr(),
                                                     d_T.data_ptr(), d_outlier.data_ptr(), d_ninl.data_ptr(), ctx.capacity, st.cuda_stream))
    st.synchronize()
    out.check(ref, nref)
    n = len(kun)
    assert np.array_equal(out.has.cpu().numpy()[:n], has_point) and np.array_equal(out.Xw.cpu().numpy()[:n], Xw)
    assert np.array_equal(d_T.cpu().numpy(), T_host) and int(d_ninl.item()) == n_host
    assert np.array_equal(d_outlier.cpu().numpy()[:n][ref >= 0], out_host[ref >= 0])
    ctx.close()
