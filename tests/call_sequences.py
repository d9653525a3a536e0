"""Scenes of tests/test_gpu_call_sequences.py: a pool of stereo pairs of UNEQUAL content at the geometry of
tests/test_gpu_plan_switches.py, the call sequences that put them through one context, and the oracle's results for every pool
image.  No extraction kernel clears its scratch, so what a call leaves behind is only harmless if every count guard holds and
every stage rewrites exactly the cells the next one reads; a sequence shows that only where a call leaves LESS behind than the
call before it: a count that shrinks, a level that empties, a row list that was over capacity and is short now.  Every pair of the
other tests' pools has the same density, so none of them does.  tests/test_call_sequences.py (CPU) pins the properties named here.

No GPU code: the device helpers at the bottom take the context and torch from their caller."""
import numpy as np

from oracle import oracle as O
from orbslam2_amd import synth

# the geometry and camera of tests/test_gpu_plan_switches.py
W, H, NF, NL = 400, 200, 400, 8
CFG = dict(width=W, height=H, nfeatures=NF, fx=350.0, fy=350.0, cx=200.0, cy=100.0, bf=140.0)

FRAMES = ("dense", "sparse", "cluster", "flat", "band", "fallback")
TEXTURED = ("dense", "band", "fallback")  # more than 20 stereo matches each; sparse and cluster match some of their few keypoints, flat has none
BAND_ROWS = (85, 115)                     # the noise band of `band`: its right row lists pass the plan's row_cap
SQUARES = ((60, 50), (200, 100), (330, 150), (120, 140))  # (x, y) of the four 12 x 12 squares of `sparse`


def _views(paint, d):
    """(left, right) of a scene that `paint(dx)` draws with its content moved dx columns to the left: the right camera sees every
    point d px further left than the left one (uR = uL - d)"""
    left, right = paint(0), paint(d)
    return np.ascontiguousarray(left), np.ascontiguousarray(right)


def _depth(d, seed):
    """the depth map of a fronto-parallel scene at disparity d, 5 % holes"""
    z = np.full((H, W), CFG["bf"] / d, np.float32)
    z[np.random.default_rng(seed).random((H, W)) < 0.05] = 0.0
    return z


def _dense():
    tex = np.random.default_rng(1).integers(0, 256, (H, W + 16), dtype=np.uint8)
    return _views(lambda dx: tex[:, dx:dx + W], 7) + (_depth(7, 11),)


def _sparse():
    def paint(dx):
        im = np.full((H, W), 90, np.uint8)
        for x, y in SQUARES:
            im[y:y + 12, x - dx:x - dx + 12] = 200
        return im
    return _views(paint, 5) + (_depth(5, 12),)


def _cluster():
    patch = np.random.default_rng(2).integers(0, 256, (40, 40), dtype=np.uint8)

    def paint(dx):
        im = np.full((H, W), 120, np.uint8)
        im[80:120, 180 - dx:220 - dx] = patch
        return im
    return _views(paint, 6) + (_depth(6, 13),)


def _flat():
    im = np.full((H, W), 77, np.uint8)
    return im, im.copy(), np.full((H, W), 2.0, np.float32)


def _band():
    r0, r1 = BAND_ROWS
    tex = np.random.default_rng(3).integers(0, 256, (r1 - r0, W + 16), dtype=np.uint8)

    def paint(dx):
        im = np.full((H, W), 120, np.uint8)
        im[r0:r1] = tex[:, dx:dx + W]
        return im
    return _views(paint, 9) + (_depth(9, 14),)


def _fallback():
    """the `low_contrast` kind of tests/test_gpu_sweep.py::test_fast_threshold_fallback_cells: most cells pass only at min_th_fast"""
    l, r, z = synth.stereo_pair(W, H, seed=91, with_depth=True, bf=CFG["bf"])
    f = lambda a: np.clip((a.astype(np.float32) - 128.0) * 0.12 + 128.0, 0, 255).astype(np.uint8)
    return f(l), f(r), z


_BUILD = dict(dense=_dense, sparse=_sparse, cluster=_cluster, flat=_flat, band=_band, fallback=_fallback)
_cache = {}


def pool():
    """name -> (left, right, depth map of the pair); built once per process"""
    if "pool" not in _cache:
        _cache["pool"] = {name: _BUILD[name]() for name in FRAMES}
    return _cache["pool"]


def row_list_lengths(kps_right, scale_factors):
    """entries of every image row's list of right keypoints as rowlist_wave counts them (vRowIndices, src/Frame.cc:474-491): keypoint
    k is listed in rows floor(y - r) .. ceil(y + r), r = 2 * scale[octave], in float32, clamped to the image"""
    rows = np.zeros(H, np.int64)
    f32 = np.float32
    for k in kps_right:
        r = f32(2.0) * f32(scale_factors[int(k["octave"])])
        lo, hi = int(np.floor(f32(k["y"]) - r)), int(np.ceil(f32(k["y"]) + r))
        rows[max(lo, 0):min(hi, H - 1) + 1] += 1
    return rows


def image_ref(ex, img, depth):
    """what the oracle gives for one image after ex.extract(img): keypoints, descriptors, per-level counts and FAST candidates,
    the blurred pyramid, and uRight / depth as an RGB-D frame of `depth`"""
    k, d = ex.extract(img)
    nl = ex.nlevels
    return dict(kps=k, desc=d, levels=[int((k["octave"] == l).sum()) for l in range(nl)],
                cand=[ex.level_candidates(l) for l in range(nl)], blur=[O.gaussian7(ex.pyramid_level(l)) for l in range(nl)],
                rgbd=O.stereo_from_rgbd(k, k, depth, CFG["bf"]), stereo=None)


def pair_refs(left, right, depth, textured, pattern=None, **kw):
    """(reference of the left image, of the right image); the left one carries the pair's uRight / depth and match count, the right
    one its row list lengths.  pattern: the rBRIEF table in force (None: the reference's)"""
    kw = dict(dict(nfeatures=NF), **kw)
    exl, exr = O.Extractor(**kw), O.Extractor(**kw)
    if pattern is not None:
        exl.set_pattern(pattern); exr.set_pattern(pattern)
    rl, rr = image_ref(exl, left, depth), image_ref(exr, right, depth)
    ur, dp, m = O.stereo_matches(exl, exr, rl["kps"], rl["desc"], rr["kps"], rr["desc"], CFG["bf"], CFG["fx"])
    assert m > 20 or not textured  # the uRight / depth comparison of a textured pair is not a comparison of empty lists
    rl["stereo"], rl["matches"] = (ur, dp), m
    rr["rows"] = row_list_lengths(rr["kps"], exr.scale_factors())
    return rl, rr


def refs():
    """(frame name, side) -> reference, side 0 the left image and 1 the right; computed once per process and never changed"""
    if "refs" not in _cache:
        out = {}
        for name, (l, r, z) in pool().items():
            out[name, 0], out[name, 1] = pair_refs(l, r, z, name in TEXTURED)
        _cache["refs"] = out
    return _cache["refs"]


def image(key):
    name, side = key
    return pool()[name][side]


def pairs(*names):
    """the slot contents of a stereo call: L0 R0 L1 R1 ..."""
    return [(n, s) for n in names for s in (0, 1)]


# ---- the sequences: steps of (entry point, slot contents); entry points stereo / extract / rgbd are the enqueue calls on device
# images, host_stereo / host_extract / host_rgbd the frame entry points on host images ----
SHRINK_GROW = [("stereo", pairs("dense", "dense", "dense")), ("stereo", pairs("sparse", "flat", "cluster")), ("stereo", pairs("flat", "flat", "flat")),
               ("stereo", pairs("band", "sparse", "dense")), ("stereo", pairs("cluster", "band", "flat"))]
FEWER_THEN_MORE = [("stereo", pairs("dense", "dense", "dense", "dense")), ("stereo", pairs("sparse")), ("stereo", pairs("flat", "band", "cluster", "dense"))]
# a slot that was a right image becomes a left or a mono one and back; every slot's keypoint count differs from the step before
PARITY = [("stereo", pairs("dense", "band")), ("extract", [("band", 1), ("sparse", 0), ("dense", 1)]),
          ("rgbd", [("cluster", 0), ("dense", 1), ("fallback", 0), ("sparse", 1)]), ("stereo", pairs("band", "cluster"))]
MIXED = [("host_stereo", pairs("dense")), ("extract", [("band", 1), ("sparse", 0), ("cluster", 0)]), ("host_extract", [("fallback", 0)]),
         ("host_rgbd", [("band", 0)]), ("stereo", pairs("sparse", "dense"))]
NO_WAIT = [("stereo", pairs("dense", "band")), ("stereo", pairs("sparse", "flat"))]


def wide_steps(n_pairs=32):
    """two stereo calls of n_pairs pairs drawn from the pool; the second gives every slot a frame of another kind"""
    n = len(FRAMES)
    first = [FRAMES[k % n] for k in range(n_pairs)]
    second = [FRAMES[(k + 1 + (k // n) % (n - 1)) % n] for k in range(n_pairs)]  # moved on by 1 .. n - 1 kinds
    assert all(a != b for a, b in zip(first, second))
    return [("stereo", pairs(*first)), ("stereo", pairs(*second))]


SEQUENCES = dict(shrink_grow=SHRINK_GROW, fewer_then_more=FEWER_THEN_MORE, parity=PARITY, mixed=MIXED, no_wait=NO_WAIT, wide=wide_steps())
CONDITIONS = ("shrunk_to_zero", "level_emptied", "level_filled", "level_equal", "level_equal_above_zero", "overflow_then_short",
              "short_then_overflow", "parity", "stale_slot")


def base_mode(mode):
    return mode.replace("host_", "")


def conditions(steps, row_cap):
    """Which stale-state conditions a sequence reaches, from the oracle's counts: per condition the (step, slot) pairs.  A slot is
    compared with what the latest call that wrote it left there.  shrunk_to_zero: the slot's keypoint count falls to 0 from above;
    level_emptied / level_filled / level_equal: a level's count of the slot falls to 0, rises from 0, stays as it was (the last also
    listed apart where it is above 0; levels that no image of the pool fills -- the last one has no quota at 400 features -- are
    left out, they are equal always); overflow_then_short / short_then_overflow: a pair's longest right row list passes row_cap in
    one call and stays within it in the next, and the other way round; parity: a slot that held a right image holds a left or a
    mono one, or the other way round; stale_slot: a slot the call before filled and this one does not"""
    R = refs()
    out = {k: [] for k in CONDITIONS}
    is_right = lambda mode, i: base_mode(mode) == "stereo" and i % 2 == 1
    live = [l for l in range(NL) if any(r["levels"][l] for r in R.values())]
    last = {}
    for s, (mode, ids) in enumerate(steps):
        if s > 0:
            out["stale_slot"] += [(s, i) for i in range(len(ids), len(steps[s - 1][1]))]
        for i, j in enumerate(ids):
            if i in last:
                m0, j0 = last[i]
                a, b = R[j0], R[j]
                if len(a["kps"]) > 0 and len(b["kps"]) == 0:
                    out["shrunk_to_zero"].append((s, i))
                for x, y in ((a["levels"][l], b["levels"][l]) for l in live):
                    for name, hit in (("level_emptied", x > 0 and y == 0), ("level_filled", x == 0 and y > 0), ("level_equal", x == y),
                                      ("level_equal_above_zero", x == y and x > 0)):
                        if hit and (s, i) not in out[name]:
                            out[name].append((s, i))
                if is_right(m0, i) != is_right(mode, i):
                    out["parity"].append((s, i))
                if is_right(m0, i) and is_right(mode, i):
                    x, y = a["rows"].max(), b["rows"].max()
                    if x > row_cap >= y:
                        out["overflow_then_short"].append((s, i))
                    if y > row_cap >= x:
                        out["short_then_overflow"].append((s, i))
            last[i] = (mode, j)
    return out


def permuted_pattern(default):
    """the reference's 256 rBRIEF tests in another order: every descriptor bit moves, no keypoint does"""
    return np.ascontiguousarray(np.asarray(default).reshape(256, 4)[np.random.default_rng(5).permutation(256)])


def frame_points(k, ur, d, nq, seed):
    """nq map points for the extracted frame (k, d, ur), as a `last frame`: keypoints drawn with replacement, back-projected at the
    identity pose (stereo depth where the keypoint has one, a random one elsewhere) and seen again from a camera 0.2 m further on"""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy, bf = (CFG[f] for f in ("fx", "fy", "cx", "cy", "bf"))
    pick = rng.integers(0, len(k), nq)
    z = np.where(ur[pick] > 0, bf / np.maximum(k["x"][pick] - ur[pick], 1e-3), rng.uniform(3.0, 30.0, nq)).astype(np.float32)
    pos = np.stack([(k["x"][pick] - cx) * z / fx, (k["y"][pick] - cy) * z / fy, z], axis=1).astype(np.float32)
    a = np.deg2rad(0.5)
    T_cur = np.array([[np.cos(a), 0, np.sin(a), 0.01], [0, 1, 0, -0.005], [-np.sin(a), 0, np.cos(a), -0.2]], np.float32)
    T_last = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(np.float32)
    return dict(pos=pos, desc=d[pick] ^ np.packbits(rng.random((nq, 256)) < 0.05, axis=1, bitorder="little"),
                valid=(rng.random(nq) < 0.9).astype(np.int32), obs=rng.integers(0, 3, nq).astype(np.int32),
                octave=k["octave"][pick].astype(np.int32), angle=((k["angle"][pick] + rng.normal(0, 5, nq)) % 360).astype(np.float32),
                T_cur=T_cur, T_last=T_last, has=(rng.random(len(k)) < 0.05).astype(np.uint8))


def camera():
    return O.Camera(CFG["fx"], CFG["fy"], CFG["cx"], CFG["cy"], CFG["bf"], CFG["bf"] / CFG["fx"])


# ---- device helpers (the caller is a GPU test) ----
def upload(torch, ids):
    return torch.from_numpy(np.stack([image(j) for j in ids])).cuda()


def upload_depth(torch, ids):
    return torch.from_numpy(np.stack([pool()[name][2] for name, _ in ids])).cuda()


def check_candidates(ctx, R, ids, what):
    """the FAST candidates of every level of every slot, in the oracle's order"""
    for i, j in enumerate(ids):
        for l in range(NL):
            for a, b in zip(ctx.fetch_candidates(i, l), R[j]["cand"][l]):
                assert np.array_equal(a, b), (what, "candidates of slot", i, j, "level", l)
