"""Call-order independence of one context.  No extraction kernel clears its scratch (orbfe_create zeroes seven
arrays once) and the context keeps host state between calls (the slot count of the latest call, its source pointer, the
matchers' grid and mvKeysUn caches, the settings), so every call starts from what the call before left.  Here one context is given
frames of UNEQUAL content in sequence (tests/call_sequences.py: counts that fall to zero and rise again, levels that empty, row
lists over capacity followed by short ones, slots that change from right image to left or mono, fewer slots then more), through
every entry point, per launch form that owns scratch of its own; settings change between calls on the same resident frame; the
matchers' grow-only scratch grows and is reused behind a call still queued.

After EVERY call every filled slot is compared with the oracle bit for bit: keypoints, descriptors, uRight and depth (through
orbfe_fetch_image and the packed block), the FAST candidates of every level, the blurred pyramid of the first and the last slot.  A
sequence's last call is then repeated alone in a fresh context and both snapshots compared byte for byte.  Every comparison is of
integers or raw bytes.  tests/test_call_sequences.py (CPU) pins which conditions each sequence reaches.

The bucket-pyramid quadtree kernel with its node tables in HBM (quadtree plan 1) is chosen from the per-level quota alone
(orbfe_plan.cpp: its LDS tables above 150 KB); no knob reaches it at 400 features, so the sequences do not run on it."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import call_sequences as S
from tests import test_matchers as TM
from tests.device_arrays import UNTOUCHED, Guarded, upload as dev_upload
from tests.plan_knobs import clear_plan_knobs
from tests.test_gpu_fast_split import SINGLE_LINE, SPLIT_LINE, snapshot
from tests.test_gpu_plan_switches import check_call

pytestmark = pytest.mark.gpu

W, H, NL = S.W, S.H, S.NL
INPLACE_LINE = "orbfe: level 0 of packed grey input: read in place (no ingest launch)"
INGEST_LINE = "orbfe: level 0 of packed grey input: copied by ingest16_kernel"
HBM_LINE = "orbfe: generic quadtree kernel: node tables in HBM scratch"
# launch form -> knobs, quadtree_plan(), quadtree_kernel(), trace lines of orbfe_create that must / must not appear
FORMS = {
    "default": ((), 0, 3, (INPLACE_LINE,), (HBM_LINE,)),
    "generic_lds": ((("ORBFE_OCTREE", "1"),), 2, 1, (INPLACE_LINE,), (HBM_LINE,)),
    "generic_hbm": ((("ORBFE_OCTREE", "2"),), 3, 1, (INPLACE_LINE, HBM_LINE), ()),
    "fast_split": ((("ORBFE_FAST_SPLIT", "1"),), 0, 3, (INPLACE_LINE,), (HBM_LINE,)),
    "no_inplace": ((("ORBFE_NO_INPLACE", "1"),), 0, 3, (INGEST_LINE,), (INPLACE_LINE, HBM_LINE)),
}


@pytest.fixture(scope="module")
def R():
    import torch  # noqa: F401  (the HIP runtime the library binds to, before the library loads)
    return S.refs()


def make_ctx(monkeypatch, capfd, form="default", max_images=8, **kw):
    """a context of launch form `form`; asserts the plan and the trace lines, so that no case silently runs the default"""
    from orbslam2_amd import api
    env, plan, kernel, present, absent = FORMS[form]
    clear_plan_knobs(monkeypatch)
    monkeypatch.delenv("ORBFE_FAST_SPLIT", raising=False)
    monkeypatch.setenv("ORBFE_HOST_TRACE", "1")
    for k, v in env:
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    ctx = api.Context(max_images=max_images, **dict(S.CFG, **kw))
    err = capfd.readouterr().err
    assert (ctx.quadtree_plan(), ctx.quadtree_kernel()) == (plan, kernel), form
    assert all(ln in err for ln in present) and not any(ln in err for ln in absent), (form, err)
    ctx.form = form
    return ctx


def check_fast_line(ctx, capfd):
    """after a context's first call: the FAST launch form it reported"""
    err = capfd.readouterr().err
    assert (SPLIT_LINE in err) != (SINGLE_LINE in err), err
    if ctx.form == "fast_split":
        assert SPLIT_LINE in err, err


def run_step(ctx, torch, R, mode, ids, stream=0, images=None):
    """one call of entry point `mode` with image ids[i] in slot i, waited for; returns what must stay alive for orbfe_fetch_pyramid"""
    from orbslam2_amd import api
    imgs = [S.image(j) for j in ids] if images is None else images
    keep = None
    if mode.startswith("host_"):
        if mode == "host_stereo":
            out = ctx.stereo_frame(imgs[0], imgs[1])
            for side, sfx in ((0, "left"), (1, "right")):
                assert out["kps_" + sfx].tobytes() == R[ids[side]]["kps"].astype(api.KP_DTYPE).tobytes(), (mode, ids)
                assert np.array_equal(out["desc_" + sfx], R[ids[side]]["desc"]), (mode, ids)
            ur, dp = R[ids[0]]["stereo"]
            assert out["u_right"].tobytes() == ur.tobytes() and out["depth"].tobytes() == dp.tobytes(), (mode, ids)
        elif mode == "host_extract":
            k, d = ctx.extract(imgs[0])
            assert k.tobytes() == R[ids[0]]["kps"].astype(api.KP_DTYPE).tobytes() and np.array_equal(d, R[ids[0]]["desc"]), (mode, ids)
        else:
            out = ctx.rgbd_frame(imgs[0], S.pool()[ids[0][0]][2])
            ur, dp = R[ids[0]]["rgbd"]
            assert out["kps"].tobytes() == R[ids[0]]["kps"].astype(api.KP_DTYPE).tobytes() and np.array_equal(out["desc"], R[ids[0]]["desc"])
            assert out["u_right"].tobytes() == ur.tobytes() and out["depth"].tobytes() == dp.tobytes(), (mode, ids)
        return keep
    dev = torch.from_numpy(np.stack(imgs)).cuda()
    keep = [dev]
    if mode == "rgbd":
        keep.append(S.upload_depth(torch, ids))
    torch.cuda.synchronize()
    if mode == "stereo":
        ctx.enqueue_stereo(dev.data_ptr(), len(ids) // 2, stream)
    elif mode == "extract":
        ctx.enqueue_extract(dev.data_ptr(), len(ids), stream)
    else:
        ctx.enqueue_rgbd(dev.data_ptr(), keep[1].data_ptr(), len(ids), stream=stream)
    ctx.synchronize(stream)
    return keep


def check_step(ctx, R, mode, ids, what):
    n = len(ids)
    check_call(ctx, R, ids, S.base_mode(mode), what, packed=not mode.startswith("host_"), blur_slots=sorted({0, n - 1}))
    S.check_candidates(ctx, R, ids, what)


def snap(ctx, mode, ids):
    return snapshot(ctx, len(ids), S.base_mode(mode) == "stereo", NL)


def run_sequence(ctx, torch, R, steps, what, capfd=None, stream_of=None, before=None, after=None):
    """every step checked against the oracle; returns the snapshot after the last one"""
    for s, (mode, ids) in enumerate(steps):
        if before:
            before(s, mode, ids)
        keep = run_step(ctx, torch, R, mode, ids, stream=stream_of(s) if stream_of else 0)
        if s == 0 and capfd is not None:
            check_fast_line(ctx, capfd)
        check_step(ctx, R, mode, ids, (what, "step %d: %s" % (s, mode), ids))
        if after:
            after(s, mode, ids, keep)
        del keep
    return snap(ctx, *steps[-1])


def alone(monkeypatch, capfd, torch, R, step, form="default", max_images=8, prepare=None):
    """the snapshot of `step` made as the first call of a fresh context of the same kind"""
    ctx = make_ctx(monkeypatch, capfd, form, max_images)
    if prepare:
        prepare(ctx)
    keep = run_step(ctx, torch, R, *step)
    out = snap(ctx, *step)
    del keep
    ctx.close()
    return out


def refused_stale_slots(ctx, api, filled, upto):
    """every fetch of a slot the latest call did not write is refused with ORBFE_ERR_INVALID before anything is read"""
    for slot in range(filled, upto):
        for fetch in (lambda: ctx.fetch_image(slot), lambda: ctx.fetch_candidates(slot, 0), lambda: ctx.fetch_keys_un(slot),
                      lambda: ctx.fetch_pyramid(slot, 0), lambda: ctx.fetch_pyramid(slot, 1, blurred=True)):
            with pytest.raises(api.OrbfeError) as e:
                fetch()
            assert e.value.code == api.ERR_INVALID and "image %d: the latest extraction call filled %d image slots" % (slot, filled) in str(e.value)
        for fetch in (lambda: ctx.fetch_packed(slot + 1, 0), lambda: ctx.fetch_counts(slot + 1)):
            with pytest.raises(api.OrbfeError) as e:
                fetch()
            assert e.value.code == api.ERR_INVALID and "the latest extraction call filled %d image slots, %d asked for" % (filled, slot + 1) in str(e.value)


# ------------------------------------------------------------------ unequal frames in sequence
@pytest.mark.parametrize("form", list(FORMS))
def test_shrink_and_grow(R, form, monkeypatch, capfd):
    """3 pairs per call: every slot's count falls, hits zero and rises; a level empties and fills again; a pair's row lists pass
    their capacity after short ones and are short after that"""
    import torch
    ctx = make_ctx(monkeypatch, capfd, form, 6)
    last = run_sequence(ctx, torch, R, S.SHRINK_GROW, form, capfd)
    ctx.close()
    assert last == alone(monkeypatch, capfd, torch, R, S.SHRINK_GROW[-1], form, 6)


@pytest.mark.parametrize("form", list(FORMS))
def test_fewer_slots_then_more(R, form, monkeypatch, capfd):
    """4 pairs -> 1 pair -> 4 pairs: the slots the middle call leaves alone still hold the first call's results, and are refused"""
    import torch
    from orbslam2_amd import api
    ctx = make_ctx(monkeypatch, capfd, form, 8)

    def after(s, mode, ids, keep):
        if s == 1:
            refused_stale_slots(ctx, api, 2, 8)

    last = run_sequence(ctx, torch, R, S.FEWER_THEN_MORE, form, capfd, after=after)
    ctx.close()
    assert last == alone(monkeypatch, capfd, torch, R, S.FEWER_THEN_MORE[-1], form, 8)


def test_parity_and_entry_point(R, monkeypatch, capfd):
    """enqueue_stereo -> enqueue_extract -> enqueue_rgbd -> enqueue_stereo: a right image's slot holds a mono image, then an RGB-D
    one, then a right image again; the RGB-D step runs on a caller stream that is not the default"""
    import torch
    ctx = make_ctx(monkeypatch, capfd, "default", 4)
    st = torch.cuda.Stream()
    last = run_sequence(ctx, torch, R, S.PARITY, "parity", capfd, stream_of=lambda s: st.cuda_stream if s == 2 else 0)
    ctx.close()
    assert last == alone(monkeypatch, capfd, torch, R, S.PARITY[-1], "default", 4)


def test_host_and_device_entry_points_mixed(R, monkeypatch, capfd):
    """stereo_frame(host) -> enqueue_extract read in place -> extract(host) -> rgbd_frame(host) -> enqueue_stereo.  Level 0 of the
    unblurred pyramid is the step's own image after a host entry point, and after an enqueue call once the caller has promised to
    keep its images; without the promise it is refused, never the image of the step before (last_src / last_src_owned)."""
    import torch
    from orbslam2_amd import api
    ctx = make_ctx(monkeypatch, capfd, "default", 4)

    def after(s, mode, ids, keep):
        own = lambda: all(np.array_equal(ctx.fetch_pyramid(i, 0), S.image(j)) for i, j in enumerate(ids))
        if mode.startswith("host_"):
            assert own(), (s, mode)
            return
        ctx.set_input_retained(0)
        with pytest.raises(api.OrbfeError) as e:
            ctx.fetch_pyramid(0, 0)
        assert e.value.code == api.ERR_UNSUPPORTED and "orbfe_set_input_retained" in str(e.value), (s, mode)
        ctx.set_input_retained(1)  # `keep` holds the call's device images
        assert own(), (s, mode)

    last = run_sequence(ctx, torch, R, S.MIXED, "mixed", capfd, after=after)
    ctx.close()
    assert last == alone(monkeypatch, capfd, torch, R, S.MIXED[-1], "default", 4)


def test_two_calls_without_a_host_wait(R, monkeypatch, capfd):
    """[dense, band] and at once [sparse, flat] on one stream: the second call's guards read counts the first call's kernels may
    not have written yet when it is enqueued; they must be read on the device, in stream order"""
    import torch
    ctx = make_ctx(monkeypatch, capfd, "default", 4)
    (m0, first), (m1, second) = S.NO_WAIT
    assert m0 == m1 == "stereo"
    d0, d1 = S.upload(torch, first), S.upload(torch, second)  # both batches are in HBM before the first call is made ...
    torch.cuda.synchronize()
    ctx.enqueue_stereo(d0.data_ptr(), len(first) // 2, 0)      # ... and nothing between the two calls blocks the host
    ctx.enqueue_stereo(d1.data_ptr(), len(second) // 2, 0)
    ctx.synchronize()
    check_step(ctx, R, m1, second, "second of two calls")
    last = snap(ctx, m1, second)
    del d0, d1
    ctx.close()
    assert last == alone(monkeypatch, capfd, torch, R, S.NO_WAIT[-1], "default", 4)


def test_stream_groups_change_between_calls(R, monkeypatch, capfd):
    """orbfe_set_streams 1 -> 3 -> 2 -> 1 -> 3 over the shrink-and-grow frames: a pair's chain moves to another stream and scratch
    region of the quadtree between calls"""
    import torch
    ctx = make_ctx(monkeypatch, capfd, "default", 6)
    groups = (1, 3, 2, 1, 3)
    last = run_sequence(ctx, torch, R, S.SHRINK_GROW, "stream groups", before=lambda s, mode, ids: ctx.set_streams(groups[s]))
    ctx.close()
    assert last == alone(monkeypatch, capfd, torch, R, S.SHRINK_GROW[-1], "default", 6, prepare=lambda c: c.set_streams(groups[-1]))


def test_unequal_frames_on_the_64_image_plan(R, monkeypatch, capfd):
    """32 pairs drawn from the pool, then 32 pairs with every slot's frame changed to another kind: every blur in FAST's launch, word
    bases from the table, the planner's own choice of the FAST split"""
    import torch
    ctx = make_ctx(monkeypatch, capfd, "default", 64)
    assert ctx.blur_ride_from(64) == 0 and ctx.blur_ride_from(63) != 0
    steps = S.SEQUENCES["wide"]
    last = run_sequence(ctx, torch, R, steps, "64 images", capfd)
    ctx.close()
    assert last == alone(monkeypatch, capfd, torch, R, steps[-1], "default", 64)


# ------------------------------------------------------------------ settings changed between calls
DIST_A = (-0.28, 0.07, 2e-4, 1e-5, 0.01)   # k1 k2 p1 p2 k3
DIST_B = (0.15, -0.05, -1e-4, 2e-4)        # k1 k2 p1 p2
FIXED_BOUNDS = (-12.0, W + 12.0, -9.0, H + 9.0)


class MatchOut:
    """the outputs of one enqueued matcher call, each between guard rows"""

    def __init__(self, cap):
        self.match, self.nm, self.status = Guarded.cells(cap), Guarded.cells(1), Guarded.cells(1)

    def result(self):
        return self.match.fetch(), int(self.nm.fetch()[0]), int(self.status.fetch()[0])

    def check(self, ref, nref, what):
        got, nm, status = self.result()
        assert status == 0 and nm == nref, (what, status, nm, nref)
        assert np.array_equal(got[: len(ref)], ref) and (got[len(ref):] == UNTOUCHED).all(), what


class LastFrame:
    """the arrays of a `last frame` in HBM, readable entries before and behind each"""

    def __init__(self, P):
        self.n = len(P["valid"])
        self.keep = [dev_upload(np.ascontiguousarray(P[f], t), front=2, pad=2) for f, t in (
            ("T_cur", np.float32), ("T_last", np.float32), ("pos", np.float32), ("desc", np.uint8), ("valid", np.int32), ("obs", np.int32),
            ("octave", np.int32), ("angle", np.float32), ("has", np.uint8))]

    def enqueue(self, ctx, bounds, th, mono, ori, out, stream):
        p = [ptr for _, ptr in self.keep]
        ctx.enqueue_search_by_projection_last(0, bounds, p[0], p[1], self.n, p[2], p[3], p[4], p[5], p[6], p[7], p[8], th, mono, ori,
                                              out.match.ptr, out.nm.ptr, out.status.ptr, stream=stream)


def test_distortion_changes_on_a_resident_frame(R, monkeypatch, capfd):
    """One stereo_frame(dense); then, with no new extraction, the coefficients A -> B -> none -> A.  After each change mvKeysUn and
    SearchByProjection(last frame) through the upload path, the resident host path and the enqueued path equal the oracle on the raw
    keypoints undistorted with THAT setting -- with the setting's own image bounds, and with one fixed set of bounds, where nothing
    but the coefficients tells a cached grid or a cached mvKeysUn from a current one.  Each path runs through all settings in a
    row: the upload path invalidates the resident host path's cache, so mixing them would hide a stale one."""
    import torch
    cam, f = S.camera(), S.CFG
    ctx = make_ctx(monkeypatch, capfd, "default", 2)
    l, r, _ = S.pool()["dense"]
    fr = ctx.stereo_frame(l, r)
    k, d, ur = fr["kps_left"], fr["desc_left"], fr["u_right"]
    assert k.tobytes() == R["dense", 0]["kps"].astype(k.dtype).tobytes()
    P = S.frame_points(k, ur, d, 300, 31)
    last = LastFrame(P)
    sf = O.Extractor(nfeatures=S.NF).scale_factors()
    st = torch.cuda.Stream()
    TH = 3.0  # px: narrow windows, so that a keypoint moved by a few px of undistortion changes its match
    settings = [("A", DIST_A), ("B", DIST_B), ("none", ()), ("A again", DIST_A)]

    def expected(dist, bounds):
        kun = k.copy()
        if len(dist):
            und = O.undistort_points(np.stack([k["x"], k["y"]], 1), f["fx"], f["fy"], f["cx"], f["cy"], dist)
            kun["x"], kun["y"] = und[:, 0], und[:, 1]
        ref, nref = O.search_by_projection_last(O.Grid(kun, *bounds), ur, d, sf, cam, P["T_cur"], P["T_last"], P["pos"], P["desc"], P["valid"],
                                                P["obs"], P["octave"], P["angle"], P["has"], TH, False, True)
        assert nref > 20
        return kun, ref, nref

    own = {}
    for name, dist in settings:  # mvKeysUn and the bounds follow the setting in force
        ctx.set_distortion(dist)
        own[name] = tuple(float(b) for b in ctx.image_bounds())
        assert own[name] == tuple(float(b) for b in O.image_bounds(W, H, f["fx"], f["fy"], f["cx"], f["cy"], np.array(dist, np.float32))), name
        assert ctx.fetch_keys_un(0).tobytes() == expected(dist, own[name])[0].tobytes(), name
    fixed = [expected(dist, FIXED_BOUNDS)[1] for _, dist in settings]
    assert not np.array_equal(fixed[0], fixed[1]) and not np.array_equal(fixed[1], fixed[2]) and not np.array_equal(fixed[2], fixed[3])
    for path in ("resident", "enqueued", "upload"):
        for which in ("fixed", "own"):
            for name, dist in settings:
                ctx.set_distortion(dist)
                bounds = FIXED_BOUNDS if which == "fixed" else own[name]
                kun, ref, nref = expected(dist, bounds)
                what = (path, which, name)
                if path == "enqueued":
                    out = MatchOut(ctx.capacity)
                    torch.cuda.synchronize()
                    last.enqueue(ctx, bounds, TH, False, True, out, st.cuda_stream)
                    st.synchronize()
                    out.check(ref, nref, what)
                    continue
                view = ctx._view(kun, ur, d, bounds, device_slot=0 if path == "resident" else None)
                got, ngot = ctx.search_by_projection_last(view, P["T_cur"], P["T_last"], P["pos"], P["desc"], P["valid"], P["obs"], P["octave"],
                                                          P["angle"], P["has"], TH, False, True)
                assert ngot == nref and np.array_equal(got, ref), what
    ctx.close()


def test_pattern_changes_between_calls(R, monkeypatch, capfd):
    """orbfe_set_pattern(permuted) and back between calls on the same images: the descriptors follow the table in force, the
    keypoints stay"""
    import torch
    ctx = make_ctx(monkeypatch, capfd, "default", 4)
    default = ctx.pattern()
    perm = S.permuted_pattern(default)
    ids = S.pairs("dense", "band")
    Rp = {}
    for name in ("dense", "band"):
        lft, rgt, z = S.pool()[name]
        Rp[name, 0], Rp[name, 1] = S.pair_refs(lft, rgt, z, True, pattern=perm)
    for j in ids:
        assert Rp[j]["kps"].tobytes() == R[j]["kps"].tobytes() and not np.array_equal(Rp[j]["desc"], R[j]["desc"])
    for what, pat, refs in (("default", None, R), ("permuted", perm, Rp), ("default again", default, R), ("permuted again", perm, Rp)):
        if pat is not None:
            ctx.set_pattern(pat)
        keep = run_step(ctx, torch, refs, "stereo", ids)
        check_step(ctx, refs, "stereo", ids, what)
        del keep
    ctx.close()


def test_input_format_changes_between_calls(R, monkeypatch, capfd):
    """1 channel -> 3 channels -> 1 channel between enqueue calls: level 0 read in place alternates with level 0 written by ingest;
    orbfe_fetch_pyramid's level 0 is the call's own grey image either way (the caller keeps its images)"""
    import torch
    ctx = make_ctx(monkeypatch, capfd, "default", 2)
    ctx.set_input_retained(1)
    P = S.pool()
    colour = [np.ascontiguousarray(np.stack([P[name][side] for name in ("dense", "band", "fallback")], axis=2)) for side in (0, 1)]
    grey = [O.cvt_gray(c, True) for c in colour]
    R2 = dict(R)
    R2["colour", 0], R2["colour", 1] = S.pair_refs(grey[0], grey[1], P["dense"][2], False)
    assert len(R2["colour", 0]["kps"]) > 100
    steps = [(1, S.pairs("sparse"), None, None), (3, S.pairs("colour"), colour, grey), (1, S.pairs("cluster"), None, None),
             (3, S.pairs("colour"), colour, grey), (1, S.pairs("dense"), None, None)]
    for s, (cn, ids, images, level0) in enumerate(steps):
        ctx.set_input_format(cn, True)
        keep = run_step(ctx, torch, R2, "stereo", ids, images=images)
        check_step(ctx, R2, "stereo", ids, ("step %d" % s, cn))
        for i, j in enumerate(ids):
            assert np.array_equal(ctx.fetch_pyramid(i, 0), S.image(j) if level0 is None else level0[i]), (s, i)
        del keep
    ctx.close()


def test_rectification_set_and_cleared_between_calls(R, monkeypatch, capfd):
    """orbfe_set_rectification on both sides, then cleared: the source size changes with it, and level 0 is the remapped image, then
    the caller's own again"""
    import torch
    from orbslam2_amd import synth
    from tests.test_gpu_parity import _rectify_maps
    ctx = make_ctx(monkeypatch, capfd, "default", 2)
    ctx.set_input_retained(1)
    sw, sh = W + 16, H + 8
    maps = [_rectify_maps(W, H, sw, sh, seed) for seed in (1, 2)]
    raw = synth.stereo_pair(sw, sh, seed=5300)
    grey = [O.remap_bilinear(im, mx, my) for im, (mx, my) in zip(raw, maps)]
    R2 = dict(R)
    R2["rect", 0], R2["rect", 1] = S.pair_refs(grey[0], grey[1], S.pool()["dense"][2], True)
    steps = [(False, S.pairs("band"), None), (True, S.pairs("rect"), list(raw)), (False, S.pairs("sparse"), None), (True, S.pairs("rect"), list(raw)),
             (False, S.pairs("dense"), None)]
    for s, (on, ids, images) in enumerate(steps):
        for side in (0, 1):
            if on:
                ctx.set_rectification(side, maps[side][0], maps[side][1], (sw, sh))
            else:
                ctx.set_rectification(side)
        keep = run_step(ctx, torch, R2, "stereo", ids, images=images)
        check_step(ctx, R2, "stereo", ids, ("step %d" % s, on))
        for i, j in enumerate(ids):
            assert np.array_equal(ctx.fetch_pyramid(i, 0), grey[i] if on else S.image(j)), (s, i)
        del keep
    ctx.close()


# ------------------------------------------------------------------ the matchers' grow-only scratch
def _resident_dense(monkeypatch, capfd, R):
    ctx = make_ctx(monkeypatch, capfd, "default", 2)
    l, r, _ = S.pool()["dense"]
    fr = ctx.stereo_frame(l, r)
    assert fr["kps_left"].tobytes() == R["dense", 0]["kps"].astype(fr["kps_left"].dtype).tobytes()
    return ctx, fr["kps_left"], fr["desc_left"], fr["u_right"]


BOUNDS = (0.0, float(W), 0.0, float(H))


def test_last_frame_queries_small_large_small(R, monkeypatch, capfd):
    """enqueue_search_by_projection_last with 8, 600 and 8 queries on one stream with no host wait: the second call frees and regrows
    the query scratch (ensure_query_scratch) behind the first, the third runs in scratch sized for the second.  All three equal the
    oracle, and the first equals its own result from a context where it ran alone."""
    import torch
    cam = S.camera()
    sf = O.Extractor(nfeatures=S.NF).scale_factors()
    alone_result = None
    for sizes in ((8, 600, 8), (8,)):
        ctx, k, d, ur = _resident_dense(monkeypatch, capfd, R)
        g = O.Grid(k, *BOUNDS)
        st = torch.cuda.Stream()
        calls = []
        for c, nq in enumerate(sizes):
            P = S.frame_points(k, ur, d, nq, 40 + c)
            ref, nref = O.search_by_projection_last(g, ur, d, sf, cam, P["T_cur"], P["T_last"], P["pos"], P["desc"], P["valid"], P["obs"],
                                                    P["octave"], P["angle"], P["has"], 15.0, False, True)
            calls.append((LastFrame(P), MatchOut(ctx.capacity), ref, nref))
        assert calls[0][3] > 0 and (len(sizes) == 1 or calls[1][3] > 100)
        torch.cuda.synchronize()
        for last, out, _, _ in calls:
            last.enqueue(ctx, BOUNDS, 15.0, False, True, out, st.cuda_stream)
        st.synchronize()
        for c, (_, out, ref, nref) in enumerate(calls):
            out.check(ref, nref, (sizes, c))
        if len(sizes) == 1:
            alone_result = calls[0][1].result()
        else:
            first = calls[0][1].result()
        ctx.close()
    assert first[1:] == alone_result[1:] and first[0].tobytes() == alone_result[0].tobytes()


def test_point_queries_small_large_small(R, monkeypatch, capfd):
    """the same for enqueue_search_by_projection_points"""
    import torch
    cam = S.camera()
    sf = O.Extractor(nfeatures=S.NF).scale_factors()
    alone_result = None
    for sizes in ((8, 600, 8), (8,)):
        ctx, k, d, ur = _resident_dense(monkeypatch, capfd, R)
        g = O.Grid(k, *BOUNDS)
        st = torch.cuda.Stream()
        calls = []
        for c, nq in enumerate(sizes):
            P = S.frame_points(k, ur, d, nq, 50 + c)
            dist0 = np.linalg.norm(P["pos"], axis=1).astype(np.float32)
            max_d = (dist0 * sf[P["octave"]]).astype(np.float32); min_d = (max_d / sf[NL - 1]).astype(np.float32)
            normal = (P["pos"] / dist0[:, None]).astype(np.float32)
            tp = O.is_in_frustum(P["T_cur"], cam, BOUNDS, P["pos"], normal, max_d, min_d, 0.5, TM.LOG_SF, NL)
            ref, nref = O.search_by_projection_points(g, ur, d, sf, tp, P["desc"], P["obs"], P["has"], 3.0, 0.8)
            dev = [dev_upload(a, front=2, pad=2) for a in (tp, P["desc"], P["obs"], P["has"])]
            calls.append((dev, nq, MatchOut(ctx.capacity), ref, nref))
        assert calls[0][4] > 0 and (len(sizes) == 1 or calls[1][4] > 100)
        torch.cuda.synchronize()
        for dev, nq, out, _, _ in calls:
            ctx.enqueue_search_by_projection_points(0, BOUNDS, nq, dev[0][1], dev[1][1], dev[2][1], 0, dev[3][1], 3.0, 0.8, out.match.ptr, out.nm.ptr,
                                                    out.status.ptr, stream=st.cuda_stream)
        st.synchronize()
        for c, (_, _, out, ref, nref) in enumerate(calls):
            out.check(ref, nref, (sizes, c))
        if len(sizes) == 1:
            alone_result = calls[0][2].result()
        else:
            first = calls[0][2].result()
        ctx.close()
    assert first[1:] == alone_result[1:] and first[0].tobytes() == alone_result[0].tobytes()
