"""The frame path at the planner's limits (tests/plan_limits.LIMITS, the table tests/test_plan_limits.py checks on the host) and on
quadtree plan 1 (octree3_kernel<true>: the bucket-pyramid kernel with its node tables in HBM scratch), HIP against the oracle.

a. both sides of every limit: a mono extract just inside and just outside (or the refusal of orbfe_create);
b. plan 1 as a subject of its own: the regimes of tests/test_gpu_quadtree_hbm.py (quota reached in the largest-first phase, fewer
   candidates than the quota, empty buckets, large and small levels in one launch, batches with stale scratch, a stereo frame);
c. the sort buffers of 8192 .. 65536 keys on plan 1 and plan 3, on the census geometries and on geometries that fill them;
d. more than 32768 keypoints per image through describe, the row lists and the stereo matcher.

Every comparison is exact (per-level candidates, keypoints as api.KP_DTYPE records, descriptors, uRight and depth), every test first
asserts the (quadtree plan, quadtree kernel) it was written for, and the oracle's own figures -- that the input reaches the edge the
case names -- are asserted beside them."""
import numpy as np
import pytest

from oracle import oracle as O
from orbslam2_amd import synth
from tests import octree_passes as P
from tests import plan_limits as PL
from tests.plan_knobs import clear_plan_knobs

pytestmark = pytest.mark.gpu

_REF = {}  # references are computed once, shared and never written to


def noise(seed, w, h, keep=1.0):
    """uniform noise; keep < 1: the columns right of that fraction of the candidate region are flat"""
    img = np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
    if keep < 1.0:
        img[:, 16 + int((w - 32) * keep):] = 128
    return img


def shifted_pair(seed, w, h, shift=11):
    """left = noise; right = the same noise `shift` px to the left plus uniform noise in [-3, 3] (an exact copy gives equal SAD
    distances, which the median cut of the stereo matcher removes)"""
    rng = np.random.default_rng(seed)
    left = rng.integers(0, 256, (h, w), dtype=np.uint8)
    right = rng.integers(0, 256, (h, w), dtype=np.uint8)
    right[:, : w - shift] = left[:, shift:]
    right = np.clip(right.astype(np.int16) + rng.integers(-3, 4, (h, w)), 0, 255).astype(np.uint8)
    return left, right


def ex_args(g):
    return dict(nfeatures=g["nfeatures"], nlevels=g["nlevels"], scale_factor=g["scale_factor"])


def mono_ref(key, g, make):
    """the oracle on make(): keypoints, descriptors, candidates of every level, the image"""
    if key not in _REF:
        img = make()
        ex = O.Extractor(**ex_args(g))
        k, d = ex.extract(img)
        _REF[key] = dict(img=img, kps=k, desc=d, cand=[ex.level_candidates(l) for l in range(g["nlevels"])])
    return _REF[key]


def stereo_ref(key, g, make, bf, fx):
    if key not in _REF:
        left, right = make()
        exl, exr = O.Extractor(**ex_args(g)), O.Extractor(**ex_args(g))
        kl, dl = exl.extract(left); kr, dr = exr.extract(right)
        ur, dp, m, bi, _ = O.stereo_matches(exl, exr, kl, dl, kr, dr, bf, fx, debug=True)
        _REF[key] = dict(left=left, right=right, kl=kl, dl=dl, kr=kr, dr=dr, ur=ur, dp=dp, m=m, best_right=bi,
                         cand=[exl.level_candidates(l) for l in range(g["nlevels"])])
    return _REF[key]


def sorted_keys(ref, g):
    """keys of the largest sort of the "largest node first" phase on level 0 (single-level geometries): its multi-point nodes"""
    xs, ys, _ = ref["cand"][0]
    passes = P.trace(xs, ys, 0, g["width"] - 32, 0, g["height"] - 32, g["nfeatures"])
    return max([p["multi"] for p in passes if p["kind"] == "sorted"], default=0)


def context(api, monkeypatch, g, expect, knobs=None, **extra):
    """a context for geometry g under g's knobs (plus `knobs`), on the (plan, kernel) the case was written for"""
    clear_plan_knobs(monkeypatch)
    kw, kn = PL.context_args(g)
    for k, v in dict(kn, **(knobs or {})).items():
        monkeypatch.setenv(k, v)
    ctx = api.Context(**kw, **extra)
    assert (ctx.quadtree_plan(), ctx.quadtree_kernel()) == expect
    return ctx


def check_mono(ctx, api, ref, image=None):
    """extract on ctx == the reference: candidates of every level, keypoints, descriptors"""
    if image is None:
        k, d = ctx.extract(ref["img"])
        image = 0
    else:
        got = ctx.fetch_image(image)
        k, d = got["kps"], got["desc"]
    for l, want in enumerate(ref["cand"]):
        for a, b in zip(ctx.fetch_candidates(image, l), want):
            assert np.array_equal(a, b), "candidates level %d" % l
    assert np.array_equal(k, ref["kps"].astype(api.KP_DTYPE)), "keypoints"
    assert np.array_equal(d, ref["desc"]), "descriptors"


def check_stereo(ctx, api, ref):
    out = ctx.stereo_frame(ref["left"], ref["right"])
    for l, want in enumerate(ref["cand"]):
        for a, b in zip(ctx.fetch_candidates(0, l), want):
            assert np.array_equal(a, b), "candidates level %d" % l
    assert np.array_equal(out["kps_left"], ref["kl"].astype(api.KP_DTYPE)), "left keypoints"
    assert np.array_equal(out["kps_right"], ref["kr"].astype(api.KP_DTYPE)), "right keypoints"
    assert np.array_equal(out["desc_left"], ref["dl"]) and np.array_equal(out["desc_right"], ref["dr"]), "descriptors"
    assert out["u_right"].tobytes() == ref["ur"].tobytes() and out["depth"].tobytes() == ref["dp"].tobytes(), "uRight / depth"
    return out


def per_level(kps, nlevels):
    return [int((kps["octave"] == l).sum()) for l in range(nlevels)]


# ---- a. both sides of every limit ----
LIMIT_SIDES = PL.sides([r for r in PL.LIMITS if not r["name"].startswith("sort_cap")])
# (candidates on level 0, keypoints) of the oracle on noise seed 31 of every accepted side
LIMIT_FIGURES = {
    "roots-inside": (619, 301), "roots-outside": (610, 301),
    "roots_level1-inside": (1392, 302), "roots_level1-outside": (1483, 303),          # per level 166 + 136 / 166 + 137
    "cells-inside": (384296, 3001), "cells-outside": (384159, 3001),
    "pyramid_tables-inside": (5926, 2379), "pyramid_tables-outside": (5926, 2379),
    "generic_tables_forced-inside": (5926, 2044),
    "generic_tables-inside": (10711, 2043), "generic_tables-outside": (10711, 2046),
    "capacity-inside": (99922, 65531),
    "capacity_8_levels-inside": (42478, 51748),                                      # levels 0 to 3 fill: 14226, 11855, 9879, 8232 of 51748
    "width-inside": (211085, 20000), "height-inside": (211153, 3004),                # largest x 32745 / largest y 32747
}


@pytest.mark.parametrize("name,row,side", LIMIT_SIDES, ids=[s[0] for s in LIMIT_SIDES])
def test_both_sides_of_every_limit(name, row, side, monkeypatch):
    from orbslam2_amd import api
    g = side["geom"]
    if side["refused"] is not None:
        clear_plan_knobs(monkeypatch)
        kw, kn = PL.context_args(g)
        for k, v in kn.items():
            monkeypatch.setenv(k, v)
        with pytest.raises(api.OrbfeError) as e:
            api.Context(**kw)
        assert e.value.code == api.ERR_UNSUPPORTED and str(e.value) == "orbfe error %d: %s" % (api.ERR_UNSUPPORTED, side["refused"])
        return
    ref = mono_ref(("limit", name), g, lambda: noise(31, g["width"], g["height"]))
    figures = (len(ref["cand"][0][0]), len(ref["kps"]))
    print(name, "level-0 candidates %d, keypoints %d, per level %s" % (figures + (per_level(ref["kps"], g["nlevels"]),)))
    assert figures == LIMIT_FIGURES[name]
    if row["name"] == "width":  # coordinates beyond what 15 bits hold minus a cell: the last root of 481
        assert ref["kps"]["x"].max() > 32700
    if row["name"] == "height":
        assert ref["kps"]["y"].max() > 32700
    ctx = context(api, monkeypatch, g, (side["plan"], side["kernel"]))
    check_mono(ctx, api, ref)
    ctx.close()


# ---- b. plan 1 ----
PLAN1 = (1, 3)
G1 = [r for r in PL.LIMITS if r["name"] == "pyramid_tables"][0]["outside"]["geom"]  # 320 x 240, one level, the first quota on HBM tables


@pytest.fixture
def plan1_ctx(monkeypatch):
    from orbslam2_amd import api
    ctx = context(api, monkeypatch, G1, PLAN1)
    yield ctx, api
    ctx.close()


def test_plan1_quota_reached_in_the_largest_first_phase(plan1_ctx):
    ctx, api = plan1_ctx
    ref = mono_ref("p1_noise", G1, lambda: noise(7, 320, 240))
    assert len(ref["cand"][0][0]) > 2 * G1["nfeatures"] and len(ref["kps"]) >= G1["nfeatures"]
    passes = P.trace(ref["cand"][0][0], ref["cand"][0][1], 0, 288, 0, 208, G1["nfeatures"])
    assert passes[-1]["kind"] == "sorted" and passes[-1]["processed"] < passes[-1]["multi"] and passes[-1]["n_out"] == len(ref["kps"])
    check_mono(ctx, api, ref)


def test_plan1_fewer_candidates_than_the_quota(plan1_ctx):
    ctx, api = plan1_ctx
    ref = mono_ref("p1_synth", G1, lambda: synth.mono_image(320, 240, seed=3))
    assert 100 < len(ref["cand"][0][0]) == len(ref["kps"]) < G1["nfeatures"]  # every candidate ends as its own node
    check_mono(ctx, api, ref)


def test_plan1_empty_buckets(plan1_ctx):
    ctx, api = plan1_ctx

    def make():
        img = noise(7, 320, 240)
        img[:, :192] = 128  # the left 60 %
        return img
    ref = mono_ref("p1_flat", G1, make)
    xs = ref["cand"][0][0]
    assert len(xs) > 1000 and xs.min() >= 192 - 16 - 3  # candidate x is relative to the 16-px border
    check_mono(ctx, api, ref)


G_MIXED = PL.geom(640, 480, 6000, nlevels=4, scale_factor=2.0)


def mixed_ref():
    ref = mono_ref("p1_mixed", G_MIXED, lambda: noise(11, 640, 480))
    quotas = O.Extractor(**ex_args(G_MIXED)).features_per_level()
    got = per_level(ref["kps"], 4)
    assert list(quotas) == [3200, 1600, 800, 400]
    assert all(got[l] >= quotas[l] for l in range(2)) and got[3] < quotas[3]  # large and small levels, and one that cannot fill
    return ref


def test_plan1_large_and_small_levels_in_one_launch(monkeypatch):
    from orbslam2_amd import api
    ref = mixed_ref()
    ctx = context(api, monkeypatch, G_MIXED, PLAN1)
    check_mono(ctx, api, ref)
    ctx.close()


@pytest.mark.parametrize("knob", ["ORBFE_NO_INPLACE", "ORBFE_NO_PROC_ORDER"])
def test_knobs_that_leave_the_quadtree_plan_alone(knob, monkeypatch):
    """the ingest copy / describe_kernel walking the slots: plan 1 on four levels, and a plan-0 row of the table on two"""
    from orbslam2_amd import api
    ref = mixed_ref()
    ctx = context(api, monkeypatch, G_MIXED, PLAN1, knobs={knob: "1"})
    check_mono(ctx, api, ref)
    ctx.close()
    side = [r for r in PL.LIMITS if r["name"] == "roots_level1"][0]["inside"]
    g = side["geom"]
    ref = mono_ref(("limit", "roots_level1-inside"), g, lambda: noise(31, g["width"], g["height"]))
    ctx = context(api, monkeypatch, g, (0, 3), knobs={knob: "1"})
    check_mono(ctx, api, ref)
    ctx.close()


G_BATCH = PL.geom(320, 240, 6100, nlevels=3)


@pytest.mark.parametrize("groups", [1, 2])
def test_plan1_batch_scratch_offsets_and_stale_scratch(groups, monkeypatch):
    """three images, three levels: every (image, level) has its own slice of the HBM scratch; the second run starts from the first
    run's scratch contents and must give the same result"""
    import torch
    from orbslam2_amd import api
    refs = [mono_ref(("p1_batch", s), G_BATCH, lambda s=s: noise(s, 320, 240)) for s in (40, 41, 42)]
    quotas = O.Extractor(**ex_args(G_BATCH)).features_per_level()
    assert quotas[0] > G1["nfeatures"] - 1 and all(per_level(r["kps"], 3)[0] >= quotas[0] for r in refs)
    ctx = context(api, monkeypatch, G_BATCH, PLAN1, max_images=3)
    ctx.set_streams(groups)
    dev = torch.from_numpy(np.stack([r["img"] for r in refs])).cuda()
    for rep in range(2):
        ctx.enqueue_extract(dev.data_ptr(), 3, 0)
        ctx.synchronize()
        for i, r in enumerate(refs):
            check_mono(ctx, api, r, image=i)
    ctx.close()


def test_plan1_stereo_frame(monkeypatch):
    """describe_kernel without the spatial processing order (plan 1 has none) feeding the row lists and the stereo matcher"""
    from orbslam2_amd import api
    fx, bf = 192.0, 80.0
    ref = stereo_ref("p1_stereo", G1, lambda: shifted_pair(50, 320, 240), bf, fx)
    print("plan 1 stereo: keypoints %d / %d, matches %d" % (len(ref["kl"]), len(ref["kr"]), ref["m"]))
    assert min(len(ref["kl"]), len(ref["kr"])) >= G1["nfeatures"] and ref["m"] > 20
    ctx = context(api, monkeypatch, G1, PLAN1, fx=fx, fy=fx, cx=160.0, cy=120.0, bf=bf)
    check_stereo(ctx, api, ref)
    ctx.close()


# ---- c. sort buffers of 8192 .. 65536 keys ----
SORT_ROWS = [(r["name"], r["inside"]["geom"], r["inside"]["sort_cap"], 1.0, False) for r in PL.LIMITS if r["name"].startswith("sort_cap")] + \
    [("sort_fill_%d" % cap, g, cap, keep, True) for g, cap, keep in PL.SORT_FILL]
# the oracle on noise seed 1: (level-0 candidates, keypoints, keys of the phase's sort)
SORT_FIGURES = {
    "sort_cap_8192": (10399, 6000, 3378), "sort_cap_16384": (22285, 12002, 4082),
    "sort_cap_32768": (36706, 20000, 8075), "sort_cap_65536": (66705, 40000, 22712),
    "sort_fill_8192": (25850, 7500, 6021), "sort_fill_16384": (51676, 15000, 12038),
    "sort_fill_32768": (82897, 30000, 23108), "sort_fill_65536": (213547, 60001, 48442),
}


@pytest.mark.parametrize("plan", [1, 3])
@pytest.mark.parametrize("name,g,cap,keep,fills", SORT_ROWS, ids=[s[0] for s in SORT_ROWS])
def test_sort_buffers_above_4096_keys(name, g, cap, keep, fills, plan, monkeypatch):
    """The "largest node first" phase ranks its multi-point nodes by a bitonic network over the power of two above their number,
    inside a buffer of `cap` keys.  The census rows sort fewer keys than half their buffer (their figures are pinned: the phase starts
    from 4^k nodes per root); the fill geometries sort more than half, i.e. run the network at the buffer's full size."""
    from orbslam2_amd import api
    ref = mono_ref(("sort", name), g, lambda: noise(1, g["width"], g["height"], keep))
    n_cand, n_kept, keys = len(ref["cand"][0][0]), len(ref["kps"]), sorted_keys(ref, g)
    print(name, "candidates %d kept %d keys %d of %d" % (n_cand, n_kept, keys, cap))
    assert (n_cand, n_kept, keys) == SORT_FIGURES[name]
    assert n_cand >= 1.5 * g["nfeatures"] and n_kept >= g["nfeatures"]
    assert cap // 2 < g["nfeatures"] + 5 <= cap  # max_nodes = quota + 5: this buffer and no smaller one
    if fills:
        assert keys > cap // 2
    ctx = context(api, monkeypatch, g, (plan, 3 if plan == 1 else 1), knobs={"ORBFE_OCTREE": "2"} if plan == 3 else None)
    check_mono(ctx, api, ref)
    ctx.close()


# ---- d. more than 32768 keypoints per image ----
@pytest.mark.parametrize("nf,slots", [(15356, 15360), (15357, 15361)])
def test_stereo_median_on_both_sides_of_its_lds_copy(nf, slots, monkeypatch):
    """stereo_median_kernel keeps a pair's SADs in 60 KB of dynamic LDS up to 15360 keypoint slots and reads them from HBM beyond
    (orbfe_launch_stereo_median; before, the launch of any larger capacity was refused by the runtime): the last capacity of the
    one form and the first of the other, both images full"""
    from orbslam2_amd import api
    g = PL.geom(640, 480, nf)
    fx, bf = 384.0, 160.0
    ref = stereo_ref(("median", nf), g, lambda: shifted_pair(70, 640, 480), bf, fx)
    print("median %d: keypoints %d / %d, matches %d" % (nf, len(ref["kl"]), len(ref["kr"]), ref["m"]))
    assert min(len(ref["kl"]), len(ref["kr"])) >= nf and ref["m"] > 1000
    ctx = context(api, monkeypatch, g, PLAN1, fx=fx, fy=fx, cx=320.0, cy=240.0, bf=bf)
    assert ctx.capacity == slots
    check_stereo(ctx, api, ref)
    ctx.close()


def test_stereo_frame_with_65531_keypoints(monkeypatch):
    """sel_total 65535: indices beyond bit 15 in the stereo keys (dist << 16 | iR, iL | cr << 16), the 16-bit row lists and
    describe_kernel's slot and order words; matches on both halves of the index range on both sides"""
    import torch
    from orbslam2_amd import api
    g = [r for r in PL.LIMITS if r["name"] == "capacity"][0]["inside"]["geom"]
    w, h = g["width"], g["height"]
    fx, bf = 0.6 * w, 0.25 * w
    ref = stereo_ref("cap_stereo", g, lambda: shifted_pair(60, w, h), bf, fx)
    matched = np.flatnonzero(ref["dp"] > 0)
    hi_left, hi_right = int((matched >= 32768).sum()), int((ref["best_right"][matched] >= 32768).sum())
    print("65531: keypoints %d / %d, matches %d, on left indices >= 32768: %d, on right indices >= 32768: %d"
          % (len(ref["kl"]), len(ref["kr"]), ref["m"], hi_left, hi_right))
    assert len(matched) == ref["m"] and min(len(ref["kl"]), len(ref["kr"])) > 65000
    assert hi_left >= 100 and hi_right >= 100
    ctx = context(api, monkeypatch, g, PLAN1, fx=fx, fy=fx, cx=w / 2, cy=h / 2, bf=bf)
    out = check_stereo(ctx, api, ref)
    assert ctx.fetch_keys_un(0).tobytes() == ref["kl"].astype(api.KP_DTYPE).tobytes()  # no distortion: the keypoints themselves
    dev = torch.from_numpy(np.stack([ref["left"], ref["right"]])).cuda()
    ctx.enqueue_stereo(dev.data_ptr(), 1, 0)
    block, lay = ctx.fetch_packed(2, api.PACK_STEREO)
    gl, gr = ctx.expand_packed(block, lay, 0), ctx.expand_packed(block, lay, 1)
    assert gl["kps"].tobytes() == out["kps_left"].tobytes() and gr["kps"].tobytes() == out["kps_right"].tobytes()
    assert np.array_equal(gl["desc"], ref["dl"]) and np.array_equal(gr["desc"], ref["dr"])
    assert gl["u_right"].tobytes() == ref["ur"].tobytes() and gl["depth"].tobytes() == ref["dp"].tobytes()
    ctx.close()


def test_eight_levels_at_the_keypoint_capacity(monkeypatch):
    """sel_total 65535 over 8 levels of 2000 x 1200: slots of every level beyond index 32768 from level 3 on"""
    from orbslam2_amd import api
    g = PL.geom(2000, 1200, 65503, nlevels=8)
    ref = mono_ref("cap8", g, lambda: noise(61, 2000, 1200))
    quotas = O.Extractor(**ex_args(g)).features_per_level()
    got = per_level(ref["kps"], 8)
    print("65503 over 8 levels: kept %d, per level %s of %s" % (len(ref["kps"]), got, list(quotas)))
    assert len(ref["kps"]) > 60000 and all(got[l] >= quotas[l] for l in range(7))
    ctx = context(api, monkeypatch, g, PLAN1)
    check_mono(ctx, api, ref)
    ctx.close()
