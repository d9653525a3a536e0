"""Scenes for the map-point update (tests/test_map_point_model.py, tests/test_map_point_device.py, tools/bench_matchers.py --map-points):
a directory of keyframes with descriptors, octaves, camera centres and bad flags, and per map point an observation list over it.
A point's descriptors are one random 256-bit base with 0..39 random bit flips per observation, so medians are close and ties common;
a point has at most one observation per keyframe, in random keyframe order (the order of mObservations is the caller's to supply).
Everything is drawn from numpy's default_rng(seed); nothing here depends on a GPU."""
import numpy as np

from tests import map_point_model as M

CENSUS_NS = (1, 2, 3, 4, 5, 8, 33, 64, 65, 130, 300)
SCALE = np.cumprod(np.concatenate([[np.float32(1)], np.full(7, np.float32(1.2))]).astype(np.float32), dtype=np.float32)  # ORBextractor's mvScaleFactor


def build(counts, n_kfs=320, kp_range=(16, 64), bad_fraction=0.15, seed=1, extra=(), extra_rows=0, permute_rows=False, scale=SCALE):
    """counts: {N: points with N observations}; extra: any of "empty" (a point without observations), "all_bad" (every observing
    keyframe bad).  extra_rows / permute_rows: a table larger than the update list, addressed through a permuted row list."""
    rng = np.random.default_rng(seed)
    kf_n = rng.integers(kp_range[0], kp_range[1] + 1, n_kfs).astype(np.int32)
    kf_bad = (rng.random(n_kfs) < bad_fraction).astype(np.int32)
    kf_bad[:4] = (1, 1, 1, 0)
    Ow = rng.uniform(-5, 5, (n_kfs, 3)).astype(np.float32)
    nlevels = len(scale)
    kf_desc = [rng.integers(0, 256, (n, 32), dtype=np.uint8) for n in kf_n]
    kf_octave = [rng.integers(0, nlevels, n).astype(np.int32) for n in kf_n]
    free = [list(rng.permutation(n)) for n in kf_n]  # slots no point has taken yet; a full keyframe shares a slot (a foreign descriptor)
    lists = [(N, None) for N, cnt in counts.items() for _ in range(cnt)] + [(0, None) for e in extra if e == "empty"] + \
            [(3, np.nonzero(kf_bad)[0]) for e in extra if e == "all_bad"]
    order = rng.permutation(len(lists))
    obs_off, obs_kf, obs_idx, ref, n_of = [0], [], [], [], []
    for li in order:
        N, pool = lists[li]
        assert N <= n_kfs
        base = rng.integers(0, 2, 256, dtype=np.uint8)
        kfs = rng.permutation(n_kfs if pool is None else pool)[:N]
        for kf in kfs:
            if free[kf]:
                idx = int(free[kf].pop())
                bits = base.copy()
                bits[rng.permutation(256)[: rng.integers(0, 40)]] ^= 1
                kf_desc[kf][idx] = np.packbits(bits)
            else:
                idx = int(rng.integers(0, kf_n[kf]))
            obs_kf.append(int(kf)); obs_idx.append(idx)
        obs_off.append(len(obs_kf))
        ref.append(int(rng.integers(0, N)) if N else 0)
        n_of.append(N)
    n_upd = len(lists)
    n_rows = n_upd + extra_rows
    row = rng.permutation(n_rows)[:n_upd].astype(np.int32) if permute_rows else None
    s = dict(kf_n=kf_n, kf_bad=kf_bad, Ow=Ow, kf_desc=kf_desc, kf_octave=kf_octave, nlevels=nlevels, scale=np.asarray(scale, np.float32),
             obs_off=np.asarray(obs_off, np.int32), obs_kf=np.asarray(obs_kf, np.int32), obs_idx=np.asarray(obs_idx, np.int32),
             ref=np.asarray(ref, np.int32), row=row, n_of=np.asarray(n_of), n_rows=n_rows,
             pos=rng.uniform(-8, 8, (n_rows, 3)).astype(np.float32))
    s["kf_desc_int"] = [[M.as_int(d) for d in kd] for kd in kf_desc]
    return s


def fresh_table(s, seed=5):
    """The table before the update: arbitrary content, so that an untouched cell is told from a written one."""
    rng = np.random.default_rng(seed)
    n = s["n_rows"]
    return dict(normal=rng.uniform(-1, 1, (n, 3)).astype(np.float32), max_d=rng.uniform(1, 9, n).astype(np.float32),
                min_d=rng.uniform(0, 1, n).astype(np.float32), desc=rng.integers(0, 256, (n, 32), dtype=np.uint8))


def census_scene():
    """The committed census scene: 200 points per N (40 from N = 130 on) over keyframes large enough that no slot is shared."""
    return build({N: (200 if N < 130 else 40) for N in CENSUS_NS}, n_kfs=320, kp_range=(400, 480), seed=11, extra=("empty", "all_bad"))


def write_scene_file(s, table, what, path):
    """The file tests/map_point_mirror/mirror_main.cpp reads."""
    first = np.concatenate([[0], np.cumsum(s["kf_n"])[:-1]]).astype(np.int32)
    n_upd = len(s["obs_off"]) - 1
    parts = [np.asarray([len(s["kf_n"]), int(s["kf_n"].sum()), n_upd, s["n_rows"], len(s["obs_kf"]), what, s["nlevels"], s["row"] is not None], np.int32),
             s["kf_n"], s["kf_bad"], first, s["Ow"], np.concatenate(s["kf_desc"]), np.concatenate(s["kf_octave"])]
    if s["row"] is not None:
        parts.append(s["row"])
    parts += [s["obs_off"], s["obs_kf"], s["obs_idx"], s["ref"], s["scale"], s["pos"], table["normal"], table["max_d"], table["min_d"], table["desc"]]
    with open(path, "wb") as f:
        for p in parts:
            f.write(np.ascontiguousarray(p).tobytes())


def read_result_file(s, path):
    """(status, best, table) as the mirror program wrote them."""
    n_upd, n = len(s["obs_off"]) - 1, s["n_rows"]
    raw = open(path, "rb").read()
    assert len(raw) == 4 + 4 * n_upd + n * (12 + 4 + 4 + 32), len(raw)
    at = [0]

    def take(dtype, count, shape):
        a = np.frombuffer(raw, dtype, count, at[0]).reshape(shape).copy()
        at[0] += a.nbytes
        return a
    status = int(take(np.int32, 1, (1,))[0])
    best = take(np.int32, n_upd, (n_upd,))
    table = dict(normal=take(np.float32, 3 * n, (n, 3)), max_d=take(np.float32, n, (n,)), min_d=take(np.float32, n, (n,)), desc=take(np.uint8, 32 * n, (n, 32)))
    return status, best, table
