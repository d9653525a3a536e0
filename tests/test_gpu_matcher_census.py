"""The census inputs of tests/matcher_census.py through the HIP entry points: for every input and every matcher it applies to, the
match array and the count equal the C oracle's exactly --

  * the synchronous entry point on a host view (every input, the scenes the suite already had included);
  * the same on the resident view (the frame injected as image slot 0 of an extraction call, device_slot=0), KeyFrame-flag views
    included;
  * the three asynchronous entry points on the resident frame: orbfe_enqueue_search_by_projection_last,
    orbfe_enqueue_is_in_frustum (field by field on the rows in view) and orbfe_enqueue_search_by_projection_points fed by the
    device's own records; nothing written beyond the frame's keypoints, status 0;
  * the overflow input on contexts of its own, so that the call under test is the one that finds the candidate list too small.

tests/test_matcher_census.py shows on the CPU what these inputs reach (points behind the camera and on its plane, both ends of the
distance range, accepted matches that a Hamming tie decides, keypoint indices above 32768, ...) and that two wrong tie rules give
other answers than the oracle on the tie inputs, which is what makes the comparisons below decisive.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import matcher_census as MC
from tests import test_matchers_device as TD
from tests.device_arrays import context, device_buffers, raw, upload

NEW = [name for name in MC.INPUTS if name not in MC.EXISTING]
KF_SIDE = ("fuse", "sim3_projection", "sim3_fuse", "by_sim3")


def hip_run(ctx, matcher, s, p, slot=None):
    """(matches, count) of the synchronous HIP entry point; slot: the current frame / keyframe is read from that image slot in HBM."""
    ur = MC._ur(s, matcher, p)
    view = ctx._view(s["k"], ur, s["d"], s["bounds"], device_slot=slot, keyframe=s["keyframe"] and matcher in KF_SIDE)
    if matcher == "last":
        return ctx.search_by_projection_last(view, s["T_cur"], s["T_last"], s["pos"], s["desc"], s["valid"], s["obs"], s["octave"], s["angle"],
                                             s["has"], p[0], p[1], p[2])
    if matcher == "points":
        tp = ctx.is_in_frustum(s["T_cur"], s["bounds"], s["pos"], s["normal"], s["max_d"], s["min_d"], 0.5)
        return ctx.search_by_projection_points(view, tp, s["desc"], s["obs"], s["has"], p[0], p[1])
    if matcher == "kf":
        return ctx.search_by_projection_kf(view, s["T_cur"], s["pos"], s["desc"], s["valid"], s["angle"], s["max_d"], s["min_d"], s["has"], p[0], p[1], p[2])
    if matcher == "fuse":
        return ctx.fuse(view, s["T_cur"], s["pos"], s["normal"], s["max_d"], s["min_d"], s["desc"], s["valid"], p[0])
    if matcher in ("sim3_projection", "sim3_fuse"):
        mode = 0 if matcher == "sim3_projection" else 1
        return ctx.sim3_projection(mode, view, s["Scw"], s["pos"], s["normal"], s["max_d"], s["min_d"], s["desc"], s["valid"],
                                   s["kf_matched"] if mode == 0 else None, p[0])
    view1 = ctx._view(s["k1"], None, s["d1"], s["bounds"], keyframe=s["keyframe"])
    return ctx.search_by_sim3(view1, s["T_last"], s["pts1"], view, s["T_cur"], s["pts2"], s["s12"], s["R12"], s["t12"], p[0])


def _inject_unfetched(ctx, k, d, ur, stream, seed=501):
    """_inject of tests/test_matchers_device.py for the SYNCHRONOUS resident view as well: the extraction call that the slot belongs to
    is enqueued and nothing of it is fetched, so the library has no host copy of the slot's keypoint count and reads the one written
    here from the device (a fetch would leave it the extraction's own count, and the view's would be refused as stale)."""
    import torch
    from orbslam2_amd import synth
    left, right = synth.stereo_pair(MC.W, MC.H, seed=seed)
    d_img = upload(np.stack([left, right]).astype(np.uint8))[0]
    torch.cuda.synchronize()
    ctx.enqueue_stereo(d_img.data_ptr(), 1, stream.cuda_stream)
    ctx.synchronize(stream.cuda_stream)
    n = len(k)
    assert n <= ctx.capacity
    b = device_buffers(ctx)
    raw(b["kps"], 28 * ctx.capacity)[: 28 * n] = upload(np.ascontiguousarray(k, O.KP_DTYPE))[0]
    raw(b["desc"], 32 * ctx.capacity)[: 32 * n] = upload(np.ascontiguousarray(d, np.uint8).reshape(-1))[0]
    raw(b["u_right"], 4 * ctx.capacity)[: 4 * n] = upload(np.ascontiguousarray(ur, np.float32).view(np.uint8))[0]
    raw(b["counts"], 4)[:] = upload(np.array([n], np.int32).view(np.uint8))[0]
    torch.cuda.synchronize()


def _same(got, ref, what):
    (g, ng), (r, nr) = got, ref
    bad = np.nonzero(g != r)[0]
    assert ng == nr and bad.size == 0, "%s: count %d vs oracle %d; differ at %s: HIP %s, oracle %s" % (
        what, ng, nr, bad[:8].tolist(), g[bad[:8]].tolist(), r[bad[:8]].tolist())


def _same_frustum(got_tp, ref_tp, what):
    assert np.array_equal(got_tp["in_view"], ref_tp["in_view"]), what
    v = ref_tp["in_view"] == 1
    for f in ("proj_x", "proj_y", "proj_xr", "level", "view_cos"):
        assert np.array_equal(got_tp[f][v], ref_tp[f][v]), (what, f)


@pytest.fixture(scope="module")
def gpu():
    from orbslam2_amd import api
    ctx = context(api)
    yield api, ctx
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,matcher", MC.CASES)
def test_gpu_census_input_on_a_host_view(gpu, name, matcher):
    api, ctx = gpu
    s, p = MC.build(name), MC.INPUTS[name][1][matcher]
    ref = MC.oracle_run(matcher, s, p)
    if matcher == "points":  # Frame::isInFrustum on the host, every row
        _same_frustum(ctx.is_in_frustum(s["T_cur"], s["bounds"], s["pos"], s["normal"], s["max_d"], s["min_d"], 0.5), MC.oracle_frustum(s), name)
    _same(hip_run(ctx, matcher, s, p), ref, "%s / %s, host view" % (name, matcher))
    _same(hip_run(ctx, matcher, s, p), ref, "%s / %s, host view, second call" % (name, matcher))


@pytest.mark.gpu
@pytest.mark.parametrize("name", NEW)
def test_gpu_census_input_on_the_resident_frame(name):
    """The input's current frame / keyframe put into image slot 0 of a context of its own (large enough for tie_wide's 34 000
    keypoints): every matcher synchronously on the resident view, then the asynchronous last / frustum / points entry points."""
    import torch
    from orbslam2_amd import api
    s = MC.build(name)
    cases = MC.INPUTS[name][1]
    nk = len(s["k"])
    ctx = context(api, nfeatures=max(2000, nk + 200))
    assert ctx.capacity >= nk
    st = torch.cuda.Stream()
    _inject_unfetched(ctx, s["k"], s["d"], s["ur"], st)
    for matcher, p in cases.items():
        ref = MC.oracle_run(matcher, s, p)
        _same(hip_run(ctx, matcher, s, p, slot=0), ref, "%s / %s, resident view" % (name, matcher))
        _same(hip_run(ctx, matcher, s, p, slot=0), ref, "%s / %s, resident view, cached grid" % (name, matcher))
    if "last" in cases:
        th, mono, ori = cases["last"]
        ref, nref = MC.oracle_run("last", s, cases["last"])
        last = TD._Last(s["T_cur"], s["T_last"], s["pos"], s["desc"], s["valid"], s["obs"], s["octave"], s["angle"], s["has"])
        for rep in range(2):
            out = TD._Out(ctx.capacity)
            torch.cuda.synchronize()
            last.enqueue(ctx, 0, s["bounds"], th, mono, ori, out, st)
            st.synchronize()
            out.check(ref, nref, "%s / enqueue last, call %d" % (name, rep))
    if "points" in cases:
        th, ratio = cases["points"]
        n = len(s["pos"])
        ref_tp = MC.oracle_frustum(s)
        ref, nref = MC.oracle_run("points", s, cases["points"])
        d_T, d_pos, d_nr, d_mx, d_mn = upload(s["T_cur"])[0], upload(s["pos"])[0], upload(s["normal"])[0], upload(s["max_d"])[0], upload(s["min_d"])[0]
        d_desc, d_obs, d_has = upload(s["desc"])[0], upload(s["obs"])[0], upload(s["has"])[0]
        d_tp = torch.zeros(n * 24, dtype=torch.uint8, device="cuda:0")
        out = TD._Out(ctx.capacity)
        torch.cuda.synchronize()
        ctx.enqueue_is_in_frustum(d_T.data_ptr(), s["bounds"], n, d_pos.data_ptr(), d_nr.data_ptr(), d_mx.data_ptr(), d_mn.data_ptr(), 0.5,
                                  d_tp.data_ptr(), st.cuda_stream)
        ctx.enqueue_search_by_projection_points(0, s["bounds"], n, d_tp.data_ptr(), d_desc.data_ptr(), d_obs.data_ptr(), 0, d_has.data_ptr(), th, ratio,
                                                out.match.data_ptr(), out.nm.data_ptr(), out.status.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        _same_frustum(d_tp.cpu().numpy().view(O.TP_DTYPE), ref_tp, "%s / enqueue frustum" % name)
        out.check(ref, nref, "%s / enqueue points" % name)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("matcher", ["fuse", "sim3_projection", "last", "points", "kf"])
def test_gpu_first_call_of_a_context_overflows_the_candidate_list(matcher):
    """run_window_queries sizes the candidate list at 64 keys per query on a context's first call and runs the kernel again when
    the windows hold more (tests/test_matcher_census.py asserts that those of this input do, with one above the 256 keys the top-K
    stage holds next to empty ones): a plain-list caller (fuse, sim3_projection) and the top-K callers, each on a fresh context --
    then once more on the list the first call left."""
    from orbslam2_amd import api
    s, p = MC.build("overflow"), MC.INPUTS["overflow"][1][matcher]
    sizes, nq = MC.window_sizes(matcher, s, p)
    assert sum(sizes) > 64 * nq and max(sizes) > 256
    ref = MC.oracle_run(matcher, s, p)
    ctx = context(api)
    _same(hip_run(ctx, matcher, s, p), ref, "overflow / %s, first call of the context" % matcher)
    _same(hip_run(ctx, matcher, s, p), ref, "overflow / %s, second call" % matcher)
    small = MC.build("tie")  # a call whose windows fit, on the grown list
    _same(hip_run(ctx, matcher, small, MC.INPUTS["tie"][1][matcher]), MC.oracle_run(matcher, small, MC.INPUTS["tie"][1][matcher]), "tie after overflow")
    ctx.close()
