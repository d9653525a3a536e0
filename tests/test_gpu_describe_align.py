"""describe_kernel's raw 31 x 31 patch through 4-byte-aligned loads (orbslam2_amd/csrc/orbfe_describe.hip): a lane loads its 16 bytes
from the 4-byte boundary below their address, o = address & 3 bytes early, and shifts them back in registers; with o >= 2 the rows
whose circle reaches u = 14 / 15 take one more aligned word.  The kernel also takes the images of a batch in the reverse of FAST's
order (xcd_map_of: reverse), whose last round is partly filled unless the image count is a multiple of 8.

Widths 160 .. 163 put the rows of level 0 read in place (pitch = width) at every misalignment, from row to row a different one
unless the width is a multiple of 4; the same widths through the pitched copy have one o per keypoint.  With a three-level pyramid
the default plan of a small batch runs the pyramid tail from level 1 and therefore copies level 0 (tests/test_describe_align_host.py
pins that), so the in-place cases set ORBFE_NO_TAIL=1.  Every slot of every call is compared with the oracle bit for bit: keypoint
records as bytes (the angle by its float bits), descriptors, and for pairs uRight / depth.  Before anything runs on the GPU the
oracle's keypoints must show every o on every level, and the crowded image keypoints on the first and last admissible column and row."""
import numpy as np
import pytest

from oracle import oracle as O
from orbslam2_amd import synth
from tests.plan_knobs import clear_plan_knobs

pytestmark = pytest.mark.gpu

H, NL, NF = 120, 3, 300
WIDTHS = (160, 161, 162, 163)
EDGE = 19
PLANS = {"in_place": {"ORBFE_NO_TAIL": "1"}, "pitched": {"ORBFE_NO_INPLACE": "1"}}
N_PAIRS = 3
FLAT, CROWDED = 2 * N_PAIRS, 2 * N_PAIRS + 1  # pool indices after the pairs' images
BATCHES = (1, 2, 3, 9)
# slot -> pool image of the extract calls: neighbouring slots differ, the flat and the crowded image are in the batch of 9 (in its
# partly filled round of the reversed map: slots 8 and 0 .. 7 are different rounds)
ORDER = (CROWDED, 0, 3, FLAT, 1, 4, 2, 5, CROWDED)


def cfg_of(w):
    return dict(width=w, height=H, nfeatures=NF, nlevels=NL, fx=140.0, fy=140.0, cx=w / 2.0, cy=H / 2.0, bf=56.0)


def crowded_image(w):
    """Bright 7 x 7 squares on a dark ground (a little noise on both, so that no two FAST scores tie), nothing else: squares whose
    outer corner pixels lie on the first and the last column and row where a keypoint may be (EDGE and size - 1 - EDGE); those
    along the last row start at every x mod 4"""
    rng = np.random.default_rng(8200 + w)
    im = rng.integers(4, 17, (H, w)).astype(np.uint8)

    def square(x0, y0):
        im[y0:y0 + 7, x0:x0 + 7] = rng.integers(238, 251, (7, 7))

    for y in (40, 60, 80):
        square(EDGE, y); square(w - 1 - EDGE - 6, y)
    for x in (34, 51, 68, 85, 102):
        square(x, EDGE); square(x, H - 1 - EDGE - 6)
    return im


def level_xy(ex, kps):
    """integer pixel of each keypoint on its own level (x = cx * scale in float32: the quotient rounds back to cx)"""
    sc = ex.scale_factors()[kps["octave"]]
    return np.rint(kps["x"] / sc).astype(np.int64), np.rint(kps["y"] / sc).astype(np.int64)


def misalignments(w, slot, ex, kps, in_place):
    """o of the first patch row (pixel (cx - 15, cy - 15)) of every keypoint, per level.  Level 0 in place: image `slot` of a packed
    batch whose first byte is 4-byte aligned, pitch w.  Pitched levels: a row starts 4 bytes into a pitch that is a multiple of 64
    and a level at a multiple of 4 from the pyramid's start (orbfe_plan.cpp: L.pitch, L.pyr_off), so o = (cx - 15) & 3."""
    cx, cy = level_xy(ex, kps)
    o = (cx - 15) & 3
    if in_place:
        o0 = (slot * w * H + (cy - 15) * w + (cx - 15)) & 3
        o = np.where(kps["octave"] == 0, o0, o)
    return {l: set(o[kps["octave"] == l].tolist()) for l in range(NL)}


@pytest.fixture(scope="module")
def pools():
    """per width: the pool's images and their oracle results, computed once"""
    out = {}
    for w in WIDTHS:
        c = cfg_of(w)
        pairs = [synth.stereo_pair(w, H, seed=8100 + 17 * k + w) for k in range(N_PAIRS)]
        images = [im for p in pairs for im in p] + [np.full((H, w), 117, np.uint8), crowded_image(w)]
        refs = []
        for im in images:
            ex = O.Extractor(nfeatures=NF, nlevels=NL)
            k, d = ex.extract(im)
            refs.append(dict(ex=ex, kps=k, desc=d, stereo=None))
        for p in range(N_PAIRS):
            l, r = refs[2 * p], refs[2 * p + 1]
            ur, dp, m = O.stereo_matches(l["ex"], r["ex"], l["kps"], l["desc"], r["kps"], r["desc"], c["bf"], c["fx"])
            assert m >= 10, (w, p, m)  # the uRight / depth comparison is not one of empty lists
            l["stereo"] = (ur, dp)
        out[w] = dict(images=images, refs=refs)
    return out


def check_inputs(w, pool, in_place):
    """CPU side: what the GPU cases are chosen for is really in them"""
    refs = pool["refs"]
    assert len(refs[FLAT]["kps"]) == 0
    seen = {l: set() for l in range(NL)}
    for slot, j in enumerate(ORDER):
        if len(refs[j]["kps"]):
            for l, s in misalignments(w, slot, refs[j]["ex"], refs[j]["kps"], in_place).items():
                seen[l] |= s
    assert all(seen[l] == {0, 1, 2, 3} for l in range(NL)), (w, seen)
    # the crowded image: keypoints on the first and last admissible column and row of level 0, and on the last admissible row one
    # with o >= 2, whose central rows take the extra word (in place, where o changes from row to row, every keypoint has such rows
    # unless the width is a multiple of 4)
    k = refs[CROWDED]["kps"]
    cx, cy = level_xy(refs[CROWDED]["ex"], k)
    l0 = k["octave"] == 0
    assert {EDGE, w - 1 - EDGE} <= set(cx[l0].tolist()) and {EDGE, H - 1 - EDGE} <= set(cy[l0].tolist()), (w, sorted(set(cx[l0].tolist())))
    if not in_place:
        last_row = l0 & (cy == H - 1 - EDGE)
        assert ((cx[last_row] - 15) & 3).max() >= 2, w


def check_slots(ctx, api, refs, ids, stereo, what):
    counts = ctx.fetch_counts(len(ids))
    for i, j in enumerate(ids):
        r = refs[j]
        with_depth = stereo and i % 2 == 0
        got = ctx.fetch_image(i, stereo=with_depth)
        assert counts[i] == len(r["kps"]), (what, i, j)
        assert got["kps"].tobytes() == r["kps"].astype(api.KP_DTYPE).tobytes(), (what, i, j)  # the angle by its float bits
        assert np.array_equal(got["desc"], r["desc"]), (what, i, j)
        if with_depth:
            ur, dp = r["stereo"]
            assert got["u_right"].tobytes() == ur.tobytes() and got["depth"].tobytes() == dp.tobytes(), (what, i, j)


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("w", WIDTHS)
def test_describe_equals_oracle_at_every_row_misalignment(pools, w, plan, monkeypatch):
    """Extract batches of 1, 2, 3 and 9 images (the flat and the crowded image among the 9) and one stereo batch of 3 pairs in one
    context, level 0 read in place or through the pitched copy."""
    import torch
    from orbslam2_amd import api
    pool = pools[w]
    check_inputs(w, pool, plan == "in_place")
    clear_plan_knobs(monkeypatch)
    for k, v in PLANS[plan].items():
        monkeypatch.setenv(k, v)
    ctx = api.Context(max_images=len(ORDER), **cfg_of(w))
    for n in BATCHES:
        ids = list(ORDER[:n])
        dev = torch.from_numpy(np.stack([pool["images"][j] for j in ids])).cuda()
        assert dev.data_ptr() % 4 == 0  # what misalignments() assumes of a packed batch
        ctx.enqueue_extract(dev.data_ptr(), n, 0)
        ctx.synchronize()
        check_slots(ctx, api, pool["refs"], ids, False, "%d %s extract %d" % (w, plan, n))
    ids = [(2 * ((p + 1) % N_PAIRS)) + s for p in range(N_PAIRS) for s in range(2)]  # pair p + 1 in slot p: new images in every slot
    dev = torch.from_numpy(np.stack([pool["images"][j] for j in ids])).cuda()
    ctx.enqueue_stereo(dev.data_ptr(), N_PAIRS, 0)
    ctx.synchronize()
    check_slots(ctx, api, pool["refs"], ids, True, "%d %s stereo" % (w, plan))
    ctx.close()
