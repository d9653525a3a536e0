"""The forms of a split pass in the bucket-pyramid quadtree kernel with LDS node tables (octree3_kernel<false>, default plan): wave 0
alone up to 64 nodes (roots, full passes, a largest-first pass), one thread per node up to 256, the general path beyond, the deep
path, and the hand-overs between them.  The images and the pass sequence each one produces are tests/octree_passes.CASES, pinned on
the CPU by tests/test_octree_passes.py.  Every comparison with the oracle is exact: keypoints as api.KP_DTYPE records, descriptors,
the level-0 candidates.  Each case runs once alone and once as a batch of all the images of its size, so that workgroups in
different regimes share compute units."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import octree_passes as P
from tests.plan_knobs import clear_plan_knobs

pytestmark = pytest.mark.gpu

BUCKET_PYRAMID_LDS = (0, 3)  # (quadtree_plan(), quadtree_kernel())


@pytest.fixture(scope="module")
def images():
    return {name: make() for name, make in P.IMAGES.items()}


@pytest.fixture(scope="module")
def reference():
    """oracle result per (image, nfeatures, nlevels), computed once"""
    cache = {}

    def get(name, img, nf, nlevels):
        key = (name, nf, nlevels)
        if key not in cache:
            ex = O.Extractor(nfeatures=nf, nlevels=nlevels)
            k, d = ex.extract(img)
            cache[key] = (k, d, [ex.level_candidates(l) for l in range(nlevels)])
        return cache[key]
    return get


def _check(api, images, reference, name, nf, nlevels=1, n_cand0=None, n_kept=None):
    import torch
    img = images[name]
    h, w = img.shape
    same_size = [n for n in images if images[n].shape == img.shape]
    ctx = api.Context(width=w, height=h, nfeatures=nf, nlevels=nlevels, max_images=len(same_size))
    try:
        assert (ctx.quadtree_plan(), ctx.quadtree_kernel()) == BUCKET_PYRAMID_LDS
        kr, dr, cands = reference(name, img, nf, nlevels)
        assert n_cand0 is None or len(cands[0][0]) == n_cand0
        assert n_kept is None or len(kr) == n_kept
        k, d = ctx.extract(img)
        for l in range(nlevels):
            for a, b in zip(ctx.fetch_candidates(0, l), cands[l]):
                assert np.array_equal(a, b), "candidates level %d" % l
        assert np.array_equal(k, kr.astype(api.KP_DTYPE)), "keypoints"
        assert np.array_equal(d, dr), "descriptors"
        dev = torch.from_numpy(np.stack([images[n] for n in same_size])).cuda()
        ctx.enqueue_extract(dev.data_ptr(), len(same_size), 0)
        ctx.synchronize()
        for i, n in enumerate(same_size):
            kb, db, _ = reference(n, images[n], nf, nlevels)
            got = ctx.fetch_image(i)
            assert np.array_equal(got["kps"], kb.astype(api.KP_DTYPE)), ("batch keypoints", n)
            assert np.array_equal(got["desc"], db), ("batch descriptors", n)
    finally:
        ctx.close()


@pytest.mark.parametrize("name,nf,n_cand,n_kept", [c[:4] for c in P.CASES], ids=["%s-%d" % (c[0], c[1]) for c in P.CASES])
def test_pass_forms(images, reference, name, nf, n_cand, n_kept, monkeypatch):
    from orbslam2_amd import api
    clear_plan_knobs(monkeypatch)
    _check(api, images, reference, name, nf, n_cand0=n_cand, n_kept=n_kept)


def test_without_the_processing_order(images, reference, monkeypatch):
    """ORBFE_NO_PROC_ORDER=1: the selection writes no describe order; the benchmark's pass sequence"""
    from orbslam2_amd import api
    clear_plan_knobs(monkeypatch)
    monkeypatch.setenv("ORBFE_NO_PROC_ORDER", "1")
    _check(api, images, reference, "noise8", 300, n_cand0=2392, n_kept=300)


def test_eight_levels_end_in_different_regimes(images, reference, monkeypatch):
    """320 x 120 noise, 1000 features on 8 levels: the levels of one launch end in different forms of pass"""
    from orbslam2_amd import api
    clear_plan_knobs(monkeypatch)
    _check(api, images, reference, "noise8", 1000, nlevels=8)
