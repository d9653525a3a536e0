"""Launch plans that the library picks per call from the number of images in a chain (orbfe_launch_pyramid, run_chain): batches
below 64 images take pair / tail kernels with word bases computed and blur beside the resize, batches of 64 and more one launch per
level with word bases from the table and every blur in FAST's launch.  One context crosses that threshold in both directions, with
new images in every slot on every call, through every batched entry point and stream grouping; the input shapes that no other test
runs at 64 images or more.  Every slot is compared with the oracle bit for bit (keypoints, descriptors, uRight, depth, and the
blurred pyramid of the slots whose pyramid is fetched).  tests/test_plan_host.py pins the plan facts these cases are chosen for."""
import numpy as np
import pytest

from oracle import oracle as O
from orbslam2_amd import synth
from tests.plan_knobs import clear_plan_knobs

pytestmark = pytest.mark.gpu

# a geometry with a three-level pyramid tail below 64 images (tests/test_plan_host.py)
W, H, NF = 400, 200, 400
CFG = dict(width=W, height=H, nfeatures=NF, fx=350.0, fy=350.0, cx=200.0, cy=100.0, bf=140.0)
ND = 3  # distinct stereo pairs: 6 distinct images; image 2 k / 2 k + 1 is pair k


def oracle_refs(pairs, kw, bf, fx, depths=None):
    """per image: keypoints, descriptors, blurred pyramid; left images: uRight / depth of their pair; with depth maps (one per pair):
    uRight / depth of every image as an RGB-D frame whose depth map is its pair's"""
    nl = kw.get("nlevels", 8)
    refs = []
    for k, (l, r) in enumerate(pairs):
        exl, exr = O.Extractor(**kw), O.Extractor(**kw)
        kl, dl = exl.extract(l); kr, dr = exr.extract(r)
        ur, dp, m = O.stereo_matches(exl, exr, kl, dl, kr, dr, bf, fx)
        assert m > 20  # the uRight / depth comparison is not a comparison of empty lists
        for kk, dd, ex, st in ((kl, dl, exl, (ur, dp)), (kr, dr, exr, None)):
            ref = dict(kps=kk, desc=dd, blur=[O.gaussian7(ex.pyramid_level(x)) for x in range(nl)], stereo=st)
            if depths is not None:
                ref["rgbd"] = O.stereo_from_rgbd(kk, kk, depths[k], bf)
            refs.append(ref)
    return refs


@pytest.fixture(scope="module")
def pool():
    import torch
    trip = [synth.stereo_pair(W, H, seed=5200 + 7 * k, with_depth=True, bf=CFG["bf"]) for k in range(ND)]
    pairs = [(l, r) for l, r, _ in trip]
    depths = [d for _, _, d in trip]
    return dict(torch=torch, pairs=pairs, depths=depths, images=[im for p in pairs for im in p],
                refs=oracle_refs(pairs, dict(nfeatures=NF), CFG["bf"], CFG["fx"], depths))


class Slots:
    """Which pool image goes into which slot: units (an image, or a pair) taken round robin from a shifted start, the shift chosen
    so that no slot receives the image it held after the latest call that wrote it, and neighbouring slots differ."""

    def __init__(self):
        self.last = {}

    def place(self, n_units, units):
        for s in range(len(units)):
            ids = [j for u in range(n_units) for j in units[(u + s) % len(units)]]
            if all(self.last.get(i) != j for i, j in enumerate(ids)):
                break
        assert all(self.last.get(i) != j for i, j in enumerate(ids)), "no shift gives every slot a new image"
        assert all(a != b for a, b in zip(ids, ids[1:]))
        self.last.update(enumerate(ids))
        return ids


IMAGES = [[j] for j in range(2 * ND)]
PAIRS = [[2 * k, 2 * k + 1] for k in range(ND)]


def check_call(ctx, refs, ids, mode, what, packed=False, blur_slots=()):
    """every slot of the latest call (mode extract / stereo / rgbd) against the oracle, through orbfe_fetch_image and, with packed,
    orbfe_fetch_batch_packed + orbfe_expand_packed; the blurred pyramid of blur_slots at every level"""
    from orbslam2_amd import api
    n = len(ids)
    counts = ctx.fetch_counts(n)
    if packed:
        block, lay = ctx.fetch_packed(n, api.PACK_STEREO if mode == "stereo" else 0)
    for i, j in enumerate(ids):
        r = refs[j]
        with_depth = mode == "rgbd" or (mode == "stereo" and i % 2 == 0)
        outs = [ctx.fetch_image(i, stereo=with_depth)] + ([ctx.expand_packed(block, lay, i)] if packed else [])
        assert counts[i] == len(r["kps"]), (what, i, j)
        for o in outs:
            assert o["kps"].tobytes() == r["kps"].astype(api.KP_DTYPE).tobytes(), (what, i, j)
            assert np.array_equal(o["desc"], r["desc"]), (what, i, j)
            if "u_right" in o:
                ur, dp = r["rgbd"] if mode == "rgbd" else r["stereo"]
                assert o["u_right"].tobytes() == ur.tobytes() and o["depth"].tobytes() == dp.tobytes(), (what, i, j)
        assert ("u_right" in outs[-1]) == (with_depth and (not packed or mode == "stereo"))
    for i in blur_slots:
        for l, b in enumerate(refs[ids[i]]["blur"]):
            assert np.array_equal(ctx.fetch_pyramid(i, l, blurred=True), b), (what, "blurred slot", i, "level", l)


def upload(torch, images, ids):
    return torch.from_numpy(np.stack([images[j] for j in ids])).cuda()


def test_extract_batch_sizes_across_the_64_image_threshold(pool, monkeypatch):
    """One context, orbfe_enqueue_extract of 1 .. 128 images in sequence: the plan switches between 63 and 64 images (and back never
    leaves a buffer from the other plan's call behind: every slot holds a new image on every call)."""
    from orbslam2_amd import api
    clear_plan_knobs(monkeypatch)
    torch, refs = pool["torch"], pool["refs"]
    ctx = api.Context(max_images=130, **CFG)
    assert ctx.blur_ride_from(63) != ctx.blur_ride_from(64) and ctx.blur_ride_from(64) == 0
    slots = Slots()
    for n in (1, 2, 3, 5, 62, 63, 64, 65, 127, 128):
        ids = slots.place(n, IMAGES)
        dev = upload(torch, pool["images"], ids)
        ctx.enqueue_extract(dev.data_ptr(), n, 0)
        ctx.synchronize()
        check_call(ctx, refs, ids, "extract", "extract %d" % n, blur_slots=sorted({0, n - 1}))
    ctx.close()


def test_stream_groups_with_chains_on_both_sides_of_the_threshold(pool, monkeypatch):
    """orbfe_set_streams cuts a batch into chains, each planned on its own size: 63 pairs in 2 groups are chains of 64 and 62 images,
    one on each plan; 65 pairs in 3 groups three small chains.  New images in every slot on every call."""
    from orbslam2_amd import api
    clear_plan_knobs(monkeypatch)
    torch, refs = pool["torch"], pool["refs"]
    ctx = api.Context(max_images=130, **CFG)
    slots = Slots()
    for pairs, groups in ((31, 1), (32, 1), (63, 2), (64, 2), (65, 3)):
        ids = slots.place(pairs, PAIRS)
        dev = upload(torch, pool["images"], ids)
        ctx.set_streams(groups)
        ctx.enqueue_stereo(dev.data_ptr(), pairs, 0)
        ctx.synchronize()
        check_call(ctx, refs, ids, "stereo", "%d pairs in %d groups" % (pairs, groups), blur_slots=(0, 2 * pairs - 1))
    ctx.close()


def test_plan_switches_across_entry_points_in_one_context(pool, monkeypatch):
    """stereo 40 pairs -> extract 7 -> stereo 3 -> RGB-D 65 -> stereo 40 -> extract 64 in one context, new images in every slot on every
    call; every result through orbfe_fetch_image and the packed block.  After a call that fills fewer slots than the one before, the
    packed fetch of the old count is refused (the stale-slot guard of orbfe_fetch_batch_packed)."""
    from orbslam2_amd import api
    clear_plan_knobs(monkeypatch)
    torch, refs = pool["torch"], pool["refs"]
    ctx = api.Context(max_images=80, **CFG)
    slots = Slots()
    depth = {j: pool["depths"][j // 2] for j in range(2 * ND)}
    prev_n = 0
    for step, (mode, units) in enumerate((("stereo", 40), ("extract", 7), ("stereo", 3), ("rgbd", 65), ("stereo", 40), ("extract", 64))):
        ids = slots.place(units, PAIRS if mode == "stereo" else IMAGES)
        n = len(ids)
        dev = upload(torch, pool["images"], ids)
        if mode == "stereo":
            ctx.enqueue_stereo(dev.data_ptr(), units, 0)
        elif mode == "extract":
            ctx.enqueue_extract(dev.data_ptr(), units, 0)
        else:
            d_depth = torch.from_numpy(np.stack([depth[j] for j in ids])).cuda()
            ctx.enqueue_rgbd(dev.data_ptr(), d_depth.data_ptr(), units)
        ctx.synchronize()
        what = "step %d: %s %d" % (step, mode, units)
        check_call(ctx, refs, ids, mode, what, packed=True, blur_slots=(0, n - 1))
        if n < prev_n:
            with pytest.raises(api.OrbfeError) as e:
                ctx.fetch_packed(prev_n, 0)
            assert e.value.code == api.ERR_INVALID and "latest extraction call filled %d image slots" % n in str(e.value), what
        prev_n = n
    ctx.close()


def _colour(pool, cn):
    """3 colour pairs whose channels are pool images (4 channels: a noise alpha, ignored by the conversion) and their grey images"""
    im = pool["images"]
    rng = np.random.default_rng(cn)
    pairs, grey = [], []
    for q in range(ND):
        side = []
        for s in range(2):
            c = np.stack([im[2 * ((q + j) % ND) + s] for j in range(3)], axis=2)  # channel j: side s of pair q + j
            if cn == 4:
                c = np.concatenate([c, rng.integers(0, 256, (H, W, 1), dtype=np.uint8)], axis=2)
            side.append(np.ascontiguousarray(c))
        pairs.append(tuple(side))
        grey.append(tuple(O.cvt_gray(c, True) for c in side))
    return pairs, grey


def _rectified(pool):
    """3 raw pairs of a larger size and their rectification maps; the grey images are the oracle's remap"""
    from tests.test_gpu_parity import _rectify_maps
    sw, sh = W + 16, H + 8
    mxl, myl = _rectify_maps(W, H, sw, sh, 1)
    mxr, myr = _rectify_maps(W, H, sw, sh, 2)
    raw = [synth.stereo_pair(sw, sh, seed=5300 + k) for k in range(ND)]
    grey = [(O.remap_bilinear(l, mxl, myl), O.remap_bilinear(r, mxr, myr)) for l, r in raw]
    return raw, grey, (mxl, myl, mxr, myr, sw, sh)


# variant -> extractor parameters, stereo pairs per call
VARIANTS = {
    "colour3": ({}, (32,)),
    "colour4": ({}, (32,)),
    "rectified": ({}, (32,)),
    "sf2.6": (dict(scale_factor=2.6, nlevels=3), (32,)),            # LDS-staged resize (pyr_resize_kernel<4>) on every level
    "patch24": (dict(patch_size=24, half_patch_size=12), (32,)),    # stereo_rowlist_kernel in a launch of its own
    "levels3": (dict(nlevels=3), (3, 32)),                          # below 64: pyr_tail_kernel<2> on levels 1-2, level 0 by ingest16_kernel
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_input_and_plan_shapes_at_64_images(pool, variant, monkeypatch):
    """Colour (3 / 4 channels) and rectified input through orbfe_enqueue_stereo, scale factor 2.6, patch size 24 and a 3-level pyramid,
    at 64 images (32 pairs) and more; the 3-level pyramid also below 64 in the same context."""
    from orbslam2_amd import api
    clear_plan_knobs(monkeypatch)
    torch = pool["torch"]
    kw, sizes = VARIANTS[variant]
    if variant.startswith("colour"):
        inputs, grey = _colour(pool, int(variant[-1]))
    elif variant == "rectified":
        inputs, grey, maps = _rectified(pool)
    else:
        inputs = grey = pool["pairs"]
    refs = oracle_refs(grey, dict(nfeatures=NF, **kw), CFG["bf"], CFG["fx"])
    images = [im for p in inputs for im in p]
    ctx = api.Context(max_images=2 * max(sizes), **CFG, **kw)
    if variant.startswith("colour"):
        ctx.set_input_format(int(variant[-1]), True)
    elif variant == "rectified":
        mxl, myl, mxr, myr, sw, sh = maps
        ctx.set_rectification(0, mxl, myl, (sw, sh))
        ctx.set_rectification(1, mxr, myr, (sw, sh))
    slots = Slots()
    for pairs in sizes:
        ids = slots.place(pairs, PAIRS)
        dev = upload(torch, images, ids)
        ctx.enqueue_stereo(dev.data_ptr(), pairs, 0)
        ctx.synchronize()
        check_call(ctx, refs, ids, "stereo", "%s %d pairs" % (variant, pairs), blur_slots=(0, 2 * pairs - 1))
    ctx.close()
