"""The generic quadtree kernel with its node tables in HBM scratch (octree_generic_kernel<true>, quadtree plan 3): the geometries
that fit neither the bucket-pyramid kernel (more than 4 roots, more than 4096 FAST cells per level) nor 150 KB of LDS node tables,
and -- forced by ORBFE_OCTREE=2 -- shapes the other kernels own.  Every comparison with the oracle is exact: keypoints as
api.KP_DTYPE records, descriptors, the per-level candidates; every case asserts the plan it was written for."""
import numpy as np
import pytest

from oracle import oracle as O
from orbslam2_amd import synth
from tests.plan_knobs import clear_plan_knobs

pytestmark = pytest.mark.gpu

GENERIC_HBM = 3
STRIP = dict(width=960, height=150, nfeatures=2200, nlevels=1)  # 8 roots; sel_cap 2204 nodes: sort buffer of 4096 keys


def _noise(seed, w, h):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def _check_mono(ctx, api, img, nfeatures, nlevels, n_kp=None, n_cand0=None, per_level=None):
    """extract on `ctx` == the oracle: candidates of every level, keypoints, descriptors; the oracle's own figures are pinned too"""
    assert ctx.quadtree_plan() == GENERIC_HBM
    k, d = ctx.extract(img)
    ex = O.Extractor(nfeatures=nfeatures, nlevels=nlevels)
    kr, dr = ex.extract(img)
    assert n_kp is None or len(kr) == n_kp
    if n_cand0 is not None:
        assert len(ex.level_candidates(0)[0]) == n_cand0
    if per_level is not None:
        assert [int((kr["octave"] == l).sum()) for l in range(nlevels)] == per_level
    for l in range(nlevels):
        for a, b in zip(ctx.fetch_candidates(0, l), ex.level_candidates(l)):
            assert np.array_equal(a, b), "candidates level %d" % l
    assert np.array_equal(k, kr.astype(api.KP_DTYPE)), "keypoints"
    assert np.array_equal(d, dr), "descriptors"
    return ex


@pytest.fixture
def strip_ctx(monkeypatch):
    from orbslam2_amd import api
    clear_plan_knobs(monkeypatch)
    ctx = api.Context(**STRIP)
    yield ctx, api
    ctx.close()


def test_quota_reached_in_the_largest_first_phase(strip_ctx):
    """A: noise, 10606 candidates in 8 roots against a quota of 2200: the sorted phase stops inside a pass (2202 nodes)."""
    ctx, api = strip_ctx
    _check_mono(ctx, api, _noise(7, 960, 150), 2200, 1, n_kp=2202, n_cand0=10606)


def test_fewer_candidates_than_the_quota(strip_ctx):
    """B: 1840 candidates: every candidate ends as its own node and the pass that adds nothing ends the loop."""
    ctx, api = strip_ctx
    _check_mono(ctx, api, synth.mono_image(960, 150, seed=3), 2200, 1, n_kp=1840, n_cand0=1840)


def test_empty_root_buckets(strip_ctx):
    """C: the left 520 columns flat: the left roots hold no candidate and are skipped."""
    ctx, api = strip_ctx
    img = _noise(7, 960, 150)
    img[:, :520] = 128
    _check_mono(ctx, api, img, 2200, 1, n_kp=2200, n_cand0=4888)


def test_eight_levels_mixed_regimes(monkeypatch):
    """D: 2048 x 256, 10000 features: levels 0 to 5 stop on the quota, level 7 has 205 candidates against a quota of 606."""
    from orbslam2_amd import api
    clear_plan_knobs(monkeypatch)
    ctx = api.Context(width=2048, height=256, nfeatures=10000)
    _check_mono(ctx, api, _noise(11, 2048, 256), 10000, 8, n_kp=9605, per_level=[2172, 1812, 1510, 1257, 1049, 873, 727, 205])
    ctx.close()


def test_4k_with_12000_features(monkeypatch):
    """E: 126 x 70 FAST cells at level 0 (beyond the bucket-pyramid kernel) and a level-0 quota beyond the LDS node tables."""
    from orbslam2_amd import api
    clear_plan_knobs(monkeypatch)
    ctx = api.Context(width=3840, height=2160, nfeatures=12000)
    _check_mono(ctx, api, synth.mono_image(3840, 2160, seed=14), 12000, 8, n_kp=12010, n_cand0=141068)
    ctx.close()


@pytest.fixture(scope="module")
def strip_batch():
    imgs = [_noise(s, 960, 150) for s in (20, 21, 22, 23)]
    ref = [O.Extractor(nfeatures=2200, nlevels=1).extract(im) for im in imgs]
    assert [len(k) for k, _ in ref] == [2200, 2202, 2202, 2200]
    return imgs, ref


@pytest.mark.parametrize("groups", [1, 2])
def test_batch_scratch_offsets_and_stale_scratch(strip_batch, groups, monkeypatch):
    """F: four images in one call: every image slot and stream group has its own scratch region; the second run of the same
    context starts from the first run's scratch contents and must give the same result."""
    import torch
    from orbslam2_amd import api
    clear_plan_knobs(monkeypatch)
    imgs, ref = strip_batch
    dev = torch.from_numpy(np.stack(imgs)).cuda()
    ctx = api.Context(max_images=4, **STRIP)
    assert ctx.quadtree_plan() == GENERIC_HBM
    ctx.set_streams(groups)
    runs = []
    for rep in range(2):
        ctx.enqueue_extract(dev.data_ptr(), 4, 0)
        ctx.synchronize()
        runs.append([ctx.fetch_image(i) for i in range(4)])
        for i, (kr, dr) in enumerate(ref):
            got = runs[rep][i]
            assert np.array_equal(got["kps"], kr.astype(api.KP_DTYPE)), (rep, i)
            assert np.array_equal(got["desc"], dr), (rep, i)
    for a, b in zip(*runs):
        assert np.array_equal(a["kps"], b["kps"]) and np.array_equal(a["desc"], b["desc"])
    ctx.close()


def _check_stereo(api, w, h, nf, left, right, nlevels=8):
    fx, bf = 0.6 * w, 0.25 * w
    ctx = api.Context(width=w, height=h, nfeatures=nf, nlevels=nlevels, fx=fx, fy=fx, cx=w / 2, cy=h / 2, bf=bf)
    assert ctx.quadtree_plan() == GENERIC_HBM
    out = ctx.stereo_frame(left, right)
    exl, exr = O.Extractor(nfeatures=nf, nlevels=nlevels), O.Extractor(nfeatures=nf, nlevels=nlevels)
    kl, dl = exl.extract(left); kr, dr = exr.extract(right)
    ur, dp, m = O.stereo_matches(exl, exr, kl, dl, kr, dr, bf, fx)
    for l in range(nlevels):
        for a, b in zip(ctx.fetch_candidates(0, l), exl.level_candidates(l)):
            assert np.array_equal(a, b), "candidates level %d" % l
    assert np.array_equal(out["kps_left"], kl.astype(api.KP_DTYPE)), "left keypoints"
    assert np.array_equal(out["kps_right"], kr.astype(api.KP_DTYPE)), "right keypoints"
    assert np.array_equal(out["desc_left"], dl) and np.array_equal(out["desc_right"], dr)
    assert np.array_equal(out["u_right"], ur) and np.array_equal(out["depth"], dp)
    ctx.close()
    return len(kl), m


# (width, height, nfeatures, seed): the golden pair, then cases of tests/test_gpu_sweep.py; shapes the bucket-pyramid kernel (or the LDS tables) own by default
FORCED = [(320, 240, 500, 1234), (200, 160, 300, 5), (96, 64, 100, 12), (64, 62, 50, 13), (410, 1000, 800, 9)]


@pytest.mark.parametrize("w,h,nf,seed", FORCED)
def test_forced_on_shapes_the_other_kernels_own(w, h, nf, seed, monkeypatch):
    """G: ORBFE_OCTREE=2 forces the HBM node tables for any geometry; stereo frame equal to the oracle."""
    from orbslam2_amd import api
    clear_plan_knobs(monkeypatch)
    monkeypatch.setenv("ORBFE_OCTREE", "2")
    left, right = synth.stereo_pair(w, h, seed=seed)
    _check_stereo(api, w, h, nf, left, right)


def test_forced_on_the_kitti_noise_image(monkeypatch):
    """G: the noise image of test_noise_image_many_candidates (more than 8192 candidates at level 0), KITTI geometry."""
    from orbslam2_amd import api
    clear_plan_knobs(monkeypatch)
    monkeypatch.setenv("ORBFE_OCTREE", "2")
    img = np.random.default_rng(99).integers(0, 256, (376, 1241)).astype(np.uint8)
    ctx = api.Context(width=1241, height=376, nfeatures=2000)
    ex = _check_mono(ctx, api, img, 2000, 8)
    assert len(ex.level_candidates(0)[0]) > 8192
    ctx.close()


def test_default_plan_of_an_owned_shape_is_not_the_hbm_form(monkeypatch):
    from orbslam2_amd import api
    clear_plan_knobs(monkeypatch)
    ctx = api.Context(width=320, height=240, nfeatures=500)
    assert ctx.quadtree_plan() == 0 and ctx.quadtree_kernel() == 3
    ctx.close()
    monkeypatch.setenv("ORBFE_OCTREE", "1")
    ctx = api.Context(width=320, height=240, nfeatures=500)
    assert ctx.quadtree_plan() == 2 and ctx.quadtree_kernel() == 1
    ctx.close()
    with pytest.raises(api.OrbfeError) as e:  # the forced LDS form keeps its refusal
        api.Context(**STRIP)
    assert e.value.code == api.ERR_UNSUPPORTED and "quadtree LDS budget" in str(e.value)


def test_stereo_frame_on_the_strip(monkeypatch):
    """H: the downstream stages (describe, row lists, stereo match) on the strip geometry's larger per-level capacity."""
    from orbslam2_amd import api
    clear_plan_knobs(monkeypatch)
    left, right = synth.stereo_pair(960, 150, seed=3)
    n, m = _check_stereo(api, 960, 150, 2200, left, right, nlevels=1)
    assert (n, m) == (1840, 856)  # the oracle's left keypoints and stereo matches
