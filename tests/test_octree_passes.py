"""tests/octree_passes.trace on the images of tests/test_gpu_octree_paths.py: the pass sequences that the GPU cases are there for
are pinned here, on the CPU, together with the oracle's candidate and keypoint counts."""
import pytest

from oracle import oracle as O
from tests import octree_passes as P


@pytest.fixture(scope="module")
def images():
    return {name: make() for name, make in P.IMAGES.items()}


@pytest.mark.parametrize("name,nf,n_cand,n_kept,chain,sorted_detail", P.CASES, ids=["%s-%d" % (c[0], c[1]) for c in P.CASES])
def test_trace_and_oracle_counts(images, name, nf, n_cand, n_kept, chain, sorted_detail):
    img = images[name]
    h, w = img.shape
    ex = O.Extractor(nfeatures=nf, nlevels=1)
    kps, _ = ex.extract(img)
    xs, ys, _ = ex.level_candidates(0)
    assert len(xs) == n_cand
    passes = P.trace(xs, ys, 0, w - 32, 0, h - 32, nf)
    assert P.chain(passes) == chain
    for i, (processed, multi) in sorted_detail.items():
        assert passes[i]["kind"] == "sorted" and (passes[i]["processed"], passes[i]["multi"]) == (processed, multi)
    assert passes[-1]["n_out"] == len(kps) == n_kept


def test_trace_ends_like_the_model():
    """the tracer's final node count is the model's keypoint count on a clustered set (one-child splits, several sorted passes)"""
    import numpy as np
    from tests import octree_model as M
    rng = np.random.default_rng(99)
    xs = np.concatenate([rng.integers(0, 12, 300), rng.integers(200, 260, 200)])
    ys = np.concatenate([rng.integers(0, 12, 300), rng.integers(40, 90, 200)])
    _, idx = np.unique(xs * 1000 + ys, return_index=True)
    xs, ys = xs[np.sort(idx)].astype(np.int32), ys[np.sort(idx)].astype(np.int32)
    sc = rng.integers(7, 255, len(xs)).astype(np.int32)
    for nf in (1, 5, 37, 100, 150, 1000):
        assert P.trace(xs, ys, 0, 300, 0, 100, nf)[-1]["n_out"] == len(M.distribute(xs, ys, sc, 0, 300, 0, 100, nf)), nf
