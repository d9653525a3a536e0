"""FAST's level 0 on the context's side stream beside the pyramid's launches (run_chain, LaunchPlan::fast_split_min_images).  Every
case runs under ORBFE_FAST_SPLIT=1, which splits at every batch size, and is compared with the oracle bit for bit and with a
context of the same kind under ORBFE_FAST_SPLIT=0 byte for byte: keypoints, descriptors, uRight, depth and the FAST candidates
of every level.  The geometry has 65 FAST cells on level 0 (13 x 5: not a multiple of the four cells of a workgroup)."""
import numpy as np
import pytest

from oracle import oracle as O
from orbslam2_amd import synth
from tests.plan_knobs import clear_plan_knobs
from tests.test_gpu_plan_switches import IMAGES, ND, PAIRS, Slots, check_call, oracle_refs, upload

pytestmark = pytest.mark.gpu

W, H, NF = 430, 200, 400
CFG = dict(width=W, height=H, nfeatures=NF, fx=350.0, fy=350.0, cx=215.0, cy=100.0, bf=140.0)
SPLIT_LINE = "orbfe: FAST: level 0 on the side stream"
SINGLE_LINE = "orbfe: FAST: one launch"


@pytest.fixture(scope="module")
def pool():
    import torch
    pairs = [synth.stereo_pair(W, H, seed=6100 + 11 * k) for k in range(ND)]
    refs = {nl: oracle_refs(pairs, dict(nfeatures=NF, nlevels=nl), CFG["bf"], CFG["fx"]) for nl in (2, 8)}
    return dict(torch=torch, pairs=pairs, images=[im for p in pairs for im in p], refs=refs)


def context(monkeypatch, split, env=(), max_images=6, **kw):
    """a context whose plan knobs are `env` and ORBFE_FAST_SPLIT=split (None: unset); the knobs are read by orbfe_create"""
    from orbslam2_amd import api
    clear_plan_knobs(monkeypatch)
    monkeypatch.setenv("ORBFE_HOST_TRACE", "1")
    for k, v in env:
        monkeypatch.setenv(k, v)
    if split is None:
        monkeypatch.delenv("ORBFE_FAST_SPLIT", raising=False)
    else:
        monkeypatch.setenv("ORBFE_FAST_SPLIT", str(split))
    return api.Context(max_images=max_images, **CFG, **kw)


def snapshot(ctx, n, stereo, nlevels):
    """everything the split may not change, as bytes, per slot"""
    out = []
    for i in range(n):
        o = ctx.fetch_image(i, stereo=stereo and i % 2 == 0)
        out.append([o[k].tobytes() for k in ("kps", "desc", "u_right", "depth") if k in o] +
                   [a.tobytes() for l in range(nlevels) for a in ctx.fetch_candidates(i, l)])
    return out


def run_both(pool, monkeypatch, capfd, mode, units, nlevels=8, env=(), stream=False, prepare=None, expect_split=True):
    """the same call on a split and an unsplit context: the split one against the oracle, then one against the other"""
    torch, refs = pool["torch"], pool["refs"][nlevels]
    ids = Slots().place(units, PAIRS if mode == "stereo" else IMAGES)
    snaps = []
    for split in (1, 0):
        capfd.readouterr()
        ctx = context(monkeypatch, split, env, max_images=max(2, len(ids)), nlevels=nlevels)
        if prepare:
            prepare(ctx)
        st = torch.cuda.Stream() if stream else None
        dev = upload(torch, pool["images"], ids)
        torch.cuda.synchronize()
        s = st.cuda_stream if st else 0
        (ctx.enqueue_stereo if mode == "stereo" else ctx.enqueue_extract)(dev.data_ptr(), units, s)
        ctx.synchronize(s)
        err = capfd.readouterr().err
        assert (SPLIT_LINE in err) == (split == 1 and expect_split) and (SINGLE_LINE in err) != (split == 1 and expect_split), err
        check_call(ctx, refs, ids, mode, "%s %d split %d" % (mode, units, split))
        snaps.append(snapshot(ctx, len(ids), mode == "stereo", nlevels))
        ctx.close()
    assert snaps[0] == snaps[1]


@pytest.mark.parametrize("nlevels", [2, 8])
@pytest.mark.parametrize("mode,units", [("extract", 1), ("extract", 3), ("stereo", 2)])
def test_split_equals_single_launch_and_oracle(pool, monkeypatch, capfd, nlevels, mode, units):
    run_both(pool, monkeypatch, capfd, mode, units, nlevels)


@pytest.mark.parametrize("ride_from", [0, 2])
def test_blur_ride_from(pool, monkeypatch, capfd, ride_from):
    """0: level 0's blur tiles ride in the side launch; 2: the pyramid's launches blur levels 0 and 1, the side launch is cells only"""
    run_both(pool, monkeypatch, capfd, "stereo", 2, env=(("ORBFE_BLUR_RIDE_FROM", str(ride_from)),))
    torch, refs = pool["torch"], pool["refs"][8]
    ctx = context(monkeypatch, 1, (("ORBFE_BLUR_RIDE_FROM", str(ride_from)),))
    ids = Slots().place(3, IMAGES)
    dev = upload(torch, pool["images"], ids)
    ctx.enqueue_extract(dev.data_ptr(), 3, 0)
    ctx.synchronize()
    check_call(ctx, refs, ids, "extract", "blurred pyramid, ride from %d" % ride_from, blur_slots=(0, 2))
    ctx.close()


def test_ingest_copy_and_colour_input(pool, monkeypatch, capfd):
    """level 0 written by ingest (the fork follows it) instead of read in place"""
    run_both(pool, monkeypatch, capfd, "stereo", 2, env=(("ORBFE_NO_INPLACE", "1"),))
    torch, im = pool["torch"], pool["images"]
    colour = [np.ascontiguousarray(np.stack([im[(j + c) % len(im)] for c in range(3)], axis=2)) for j in range(3)]
    grey = [O.cvt_gray(c, True) for c in colour]
    want = []
    for g in grey:
        ex = O.Extractor(nfeatures=NF)
        want.append(ex.extract(g))
    snaps = []
    for split in (1, 0):
        from orbslam2_amd import api
        ctx = context(monkeypatch, split)
        ctx.set_input_format(3, True)
        dev = torch.from_numpy(np.stack(colour)).cuda()
        ctx.enqueue_extract(dev.data_ptr(), 3, 0)
        ctx.synchronize()
        for i, (kk, dd) in enumerate(want):
            o = ctx.fetch_image(i)
            assert o["kps"].tobytes() == kk.astype(api.KP_DTYPE).tobytes() and np.array_equal(o["desc"], dd), (split, i)
        snaps.append(snapshot(ctx, 3, False, 8))
        ctx.close()
    assert snaps[0] == snaps[1] and SPLIT_LINE in capfd.readouterr().err


def test_caller_stream_that_is_not_the_default(pool, monkeypatch, capfd):
    run_both(pool, monkeypatch, capfd, "stereo", 2, stream=True)


def test_two_calls_without_synchronisation(pool, monkeypatch, capfd):
    """different images in every slot, the second call queued straight behind the first: a join left over from the first call
    would let the second call's quadtree run before its own level-0 cells"""
    torch, refs = pool["torch"], pool["refs"][8]
    snaps = []
    for split in (1, 0):
        ctx = context(monkeypatch, split)
        slots = Slots()
        first, second = slots.place(3, PAIRS), slots.place(3, PAIRS)
        assert all(a != b for a, b in zip(first, second))
        d1, d2 = upload(torch, pool["images"], first), upload(torch, pool["images"], second)
        torch.cuda.synchronize()
        ctx.enqueue_stereo(d1.data_ptr(), 3, 0)
        ctx.enqueue_stereo(d2.data_ptr(), 3, 0)
        ctx.synchronize()
        check_call(ctx, refs, second, "stereo", "second of two calls, split %d" % split)
        snaps.append(snapshot(ctx, 6, True, 8))
        ctx.close()
    assert snaps[0] == snaps[1] and SPLIT_LINE in capfd.readouterr().err


def test_profiled_context_keeps_the_single_launch(pool, monkeypatch, capfd):
    """stage events time the caller's stream only: with profiling on, ORBFE_FAST_SPLIT=1 still runs one FAST launch"""
    run_both(pool, monkeypatch, capfd, "stereo", 2, prepare=lambda ctx: ctx.set_profiling(1), expect_split=False)


def test_stream_groups_keep_the_single_launch(pool, monkeypatch, capfd):
    run_both(pool, monkeypatch, capfd, "stereo", 3, prepare=lambda ctx: ctx.set_streams(2), expect_split=False)


def test_default_plan_at_64_images(pool, monkeypatch, capfd):
    """no knob: the planner's own choice for a batch of 64 images, and for the 3 images that follow in the same context"""
    torch, refs = pool["torch"], pool["refs"][8]
    ctx = context(monkeypatch, None, max_images=64)
    slots = Slots()
    for n in (64, 3):
        ids = slots.place(n, IMAGES)
        dev = upload(torch, pool["images"], ids)
        capfd.readouterr()
        ctx.enqueue_extract(dev.data_ptr(), n, 0)
        ctx.synchronize()
        err = capfd.readouterr().err
        # whatever the planner's threshold is, it reports its choice, and never splits a batch below the one from which every blur rides
        assert n != 64 or (SPLIT_LINE in err) != (SINGLE_LINE in err), err  # the first call of a context always reports
        assert SPLIT_LINE not in err or ctx.blur_ride_from(n) == 0, err
        check_call(ctx, refs, ids, "extract", "default plan, %d images" % n)
    ctx.close()
