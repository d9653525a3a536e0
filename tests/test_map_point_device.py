"""orbfe_enqueue_update_map_points (orbslam2_amd/csrc/orbfe_map_point_device.hip): MapPoint::ComputeDistinctiveDescriptors and
MapPoint::UpdateNormalAndDepth for rows of the map-point table in HBM.  Every comparison is exact -- descriptor bytes and float bits --
against the literal model (tests/map_point_model.py), which tests/test_map_point_model.py plays against the C++ host mirror.

Device arrays are torch tensors.  Every input carries FRONT entries before and PAD entries behind its payload (a check the kernel
misses then reads inside the test's own allocation and shows as a wrong status or result: the padding of the keyframe directory is a
copy of a real record, not zeros); every output is surrounded by GUARD sentinel rows; the stream is never the default one."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import map_point_model as M
from tests import map_point_scenes as S
from tests import matcher_census as MC
from tests import test_fuse_device as TF
from tests.device_arrays import Guarded, context, upload

NAME = "orbfe_enqueue_update_map_points"
FRONT, PAD = 64, 64
SCALE = O.Extractor().scale_factors()
GPU_NS = {1: 6, 2: 6, 3: 6, 4: 6, 5: 6, 8: 6, 33: 4, 63: 4, 64: 4, 65: 4, 130: 3, 300: 2}
_cache = {}


def _scene(rows):
    """The scene of the exact comparison: N in GPU_NS over 320 keyframes of 16..64 keypoints, some bad, an empty and an all-bad list;
    rows = "list": a permuted row list into a table 21 rows larger than the update count."""
    if rows not in _cache:
        _cache[rows] = S.build(GPU_NS, n_kfs=320, kp_range=(16, 64), seed=21, extra=("empty", "all_bad"), scale=SCALE,
                               extra_rows=21 if rows == "list" else 0, permute_rows=rows == "list")
    return _cache[rows]


def _expected(rows, what):
    key = (rows, what)
    if key not in _cache:
        s = _scene(rows)
        table = S.fresh_table(s)
        best, status = M.update_map_points(s, what, table)
        _cache[key] = (table, best, status)
    return _cache[key]


# ------------------------------------------------------------------ CPU
def _args(**kw):
    """A call that passes every check the arguments alone allow (the pointers are never followed without a context)."""
    a = dict(ctx=None, d_kfs=8, n_kfs=2, n_upd=3, d_row=8, n_rows=3, d_obs_off=8, d_obs_kf=8, d_obs_idx=8, n_obs=5, d_ref=8, what=3, d_pos=8,
             d_normal=8, d_max_distance=8, d_min_distance=8, d_pt_desc=8, d_best=8, d_status=8, stream=None)
    a.update(kw)
    return [a[k] or None if k.startswith("d_") else a[k] for k in a]


REFUSED = [
    (dict(d_status=0), "null d_status"),
    (dict(n_kfs=-1), "negative count"), (dict(n_upd=-1), "negative count"), (dict(n_rows=-1), "negative count"), (dict(n_obs=-1), "negative count"),
    (dict(what=0), "what = 0"), (dict(what=4), "what = 4"), (dict(what=-1), "what = -1"),
    (dict(d_row=0, n_rows=2), "without a row list"),
    (dict(d_obs_off=0), "null d_obs_off or d_pos"), (dict(d_pos=0), "null d_obs_off or d_pos"), (dict(d_pos=0, what=1), "null d_obs_off or d_pos"),
    (dict(d_pt_desc=0), "null descriptor column"), (dict(d_pt_desc=0, what=1), "null descriptor column"),
    (dict(d_normal=0), "null normal or distance column"), (dict(d_max_distance=0, what=2), "null normal or distance column"),
    (dict(d_min_distance=0), "null normal or distance column"),
    (dict(d_ref=0), "null d_ref"), (dict(d_ref=0, what=2), "null d_ref"),
    (dict(d_kfs=0), "null keyframe directory"), (dict(d_obs_kf=0), "null keyframe directory"), (dict(d_obs_idx=0), "null keyframe directory"),
]
# not refused by the arguments: only the missing context is
ALLOWED = [dict(), dict(d_best=0), dict(d_row=0), dict(d_row=8, n_rows=0), dict(what=1, d_normal=0, d_max_distance=0, d_min_distance=0, d_ref=0),
           dict(what=2, d_pt_desc=0), dict(n_obs=0, d_kfs=0, d_obs_kf=0, d_obs_idx=0), dict(n_upd=0, d_obs_off=0, d_pos=0, d_pt_desc=0, d_ref=0)]


def test_the_library_exports_the_call_and_the_keyframe_record():
    from orbslam2_amd import api
    L = api.load()
    assert NAME in api.EXPORTS
    fn = getattr(L, NAME)  # AttributeError: the symbol is not exported
    assert fn(*[0 if t is C.c_int else None for t in fn.argtypes]) == api.ERR_INVALID
    assert callable(api.Context.enqueue_update_map_points)
    assert C.sizeof(api.ObsKeyframe) == 40 and api.OBS_KF_DTYPE.itemsize == 40
    assert [(n, api.OBS_KF_DTYPE.fields[n][1]) for n, _ in api.ObsKeyframe._fields_] == [(n, getattr(api.ObsKeyframe, n).offset) for n, _ in api.ObsKeyframe._fields_]
    assert (api.MP_DESCRIPTOR, api.MP_NORMAL_DEPTH) == (1, 2) == (M.MP_DESCRIPTOR, M.MP_NORMAL_DEPTH)


def test_what_the_arguments_alone_show_is_refused_before_anything_else():
    """Without a device there is no context, and a NULL context is refused too -- so the refusals are told apart by the message."""
    from orbslam2_amd import api
    L = api.load()
    fn = getattr(L, NAME)
    for kw, message in REFUSED:
        assert fn(*_args(**kw)) == api.ERR_INVALID, kw
        assert message in L.orbfe_last_error(None).decode(), (kw, L.orbfe_last_error(None))
    for kw in ALLOWED:
        assert fn(*_args(**kw)) == api.ERR_INVALID, kw
        assert L.orbfe_last_error(None) == b"null context", (kw, L.orbfe_last_error(None))


def test_the_scene_reaches_every_path_of_the_kernel():
    s = _scene("list")
    n_upd = len(s["n_of"])
    assert n_upd % 4 and n_upd > 8                      # the last workgroup is not full, and there is more than one
    assert set(GPU_NS) <= set(s["n_of"].tolist()) and 0 in s["n_of"]
    assert s["kf_n"].min() >= 16 and s["kf_n"].max() <= 64 and len(s["kf_n"]) == 320 and 0 < s["kf_bad"].sum() < 320
    assert s["n_rows"] > n_upd and len(set(s["row"].tolist())) == n_upd and not np.array_equal(s["row"], np.arange(n_upd))
    table, best, status = _expected("list", 3)
    ignoring, _ = M.update_map_points(s, 1, S.fresh_table(s), ignore_bad=True)
    big = s["n_of"] > 64
    assert status == 0 and (best[big] > 63).any()       # a winner in a later block of 64 rows
    assert (best[s["n_of"] >= 3] > 0).any() and (best != ignoring).any() and (best[big] != ignoring[big]).any()
    # a list of more than 64 entries of which no more than 64 are good, and one whose good count stays above 64
    good = np.array([sum(1 - s["kf_bad"][s["obs_kf"][o]] for o in range(s["obs_off"][q], s["obs_off"][q + 1])) for q in range(n_upd)])
    assert ((s["n_of"] == 65) & (good <= 64)).any() and (good > 64).any()
    assert ((s["n_of"] == 3) & (good == 0)).any()


# ------------------------------------------------------------------ helpers (GPU)
class _Device:
    """A scene in HBM: the keyframe directory (one descriptor and one keypoint buffer, records into them) and the observation lists."""

    def __init__(self, api, s):
        self.s, self.api = s, api
        first = np.concatenate([[0], np.cumsum(s["kf_n"])[:-1]]).astype(np.int64)
        keys = np.zeros(int(s["kf_n"].sum()), O.KP_DTYPE)
        keys["octave"] = np.concatenate(s["kf_octave"])
        self.desc, desc_ptr = upload(np.concatenate(s["kf_desc"]), FRONT, PAD)
        self.keys, keys_ptr = upload(keys, FRONT, PAD)
        rec = np.zeros(len(s["kf_n"]), api.OBS_KF_DTYPE)
        rec["desc"], rec["keys_un"] = desc_ptr + 32 * first, keys_ptr + O.KP_DTYPE.itemsize * first
        rec["Ow"], rec["n"], rec["bad"] = s["Ow"], s["kf_n"], s["kf_bad"]
        self.rec, self.rec_ptr = upload(rec, FRONT, PAD, fill=rec[len(rec) // 2])
        self.lists = {k: upload(s[k], FRONT, PAD) for k in ("obs_off", "obs_kf", "obs_idx", "ref")}
        self.row = None if s["row"] is None else upload(s["row"], FRONT, PAD)
        self.pos = upload(s["pos"], FRONT, PAD)

    def run(self, ctx, stream, what, table, with_best=True):
        """Queues the update of `table` (numpy columns) on `stream`; returns (status, best or None, the table as the device left it)."""
        import torch
        s = self.s
        n_upd = len(s["obs_off"]) - 1
        cols = {k: Guarded(table[k]) for k in ("normal", "max_d", "min_d", "desc")}
        best, status = Guarded.cells(n_upd), Guarded.cells(1)
        torch.cuda.synchronize()  # the uploads and fills above ran on torch's own stream
        ctx.enqueue_update_map_points(self.rec_ptr, len(s["kf_n"]), n_upd, 0 if self.row is None else self.row[1], s["n_rows"], self.lists["obs_off"][1],
                                      self.lists["obs_kf"][1], self.lists["obs_idx"][1], len(s["obs_kf"]), self.lists["ref"][1], what, self.pos[1],
                                      cols["normal"].ptr, cols["max_d"].ptr, cols["min_d"].ptr, cols["desc"].ptr,
                                      best.ptr if with_best else 0, status.ptr, stream=stream.cuda_stream)
        stream.synchronize()
        if not with_best:
            assert best.untouched()
        return int(status.fetch()[0]), best.fetch() if with_best else None, {k: c.fetch() for k, c in cols.items()}


def _same(got, want, what):
    for k in want:
        a, b = np.ascontiguousarray(got[k]).view(np.uint8).reshape(len(want[k]), -1), np.ascontiguousarray(want[k]).view(np.uint8).reshape(len(want[k]), -1)
        rows = np.nonzero((a != b).any(axis=1))[0]
        assert rows.size == 0, "%s: column %s differs in rows %s: device %s, model %s" % (what, k, rows[:6].tolist(), got[k][rows[:3]].tolist(),
                                                                                     want[k][rows[:3]].tolist())


@pytest.fixture(scope="module")
def gpu():
    import torch
    from orbslam2_amd import api
    ctx = context(api)
    assert np.array_equal(ctx.tables()["scale"], SCALE) and ctx.nlevels == len(SCALE)
    devices = {}

    def device_of(rows):
        if rows not in devices:
            devices[rows] = _Device(api, _scene(rows))
            torch.cuda.synchronize()
        return devices[rows]
    yield api, ctx, torch.cuda.Stream(), device_of
    ctx.close()


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("rows", ["null", "list"])
@pytest.mark.parametrize("what", [1, 2, 3])
def test_gpu_update_equals_the_model_exactly(gpu, what, rows):
    """Descriptor bytes and float bits of every row; the columns `what` does not select, the rows no update names, the rows of the empty
    list and (descriptor) of the all-bad list come back as they were uploaded."""
    api, ctx, st, device_of = gpu
    s, dev = _scene(rows), device_of(rows)
    want, want_best, want_status = _expected(rows, what)
    before = S.fresh_table(s)
    for call in range(2):  # the second call: no state is kept between calls
        status, best, got = dev.run(ctx, st, what, before)
        assert status == want_status == 0
        assert np.array_equal(best, want_best), (np.nonzero(best != want_best)[0][:8], best[best != want_best][:8], want_best[best != want_best][:8])
        _same(got, want, "what = %d, rows = %s, call %d" % (what, rows, call))
    unselected = [k for k, bit in (("desc", 1), ("normal", 2), ("max_d", 2), ("min_d", 2)) if not what & bit]
    assert all(np.array_equal(want[k], before[k]) for k in unselected) and len(unselected) == (0 if what == 3 else 3 if what == 1 else 1)
    if what == 3:
        written = {k: (want[k] != before[k]).reshape(len(before[k]), -1).any(axis=1) for k in want}
        named = np.zeros(s["n_rows"], bool)
        named[s["row"] if s["row"] is not None else np.arange(len(s["n_of"]))] = True
        assert not (written["normal"] & ~named).any() and written["normal"].sum() == len(s["n_of"]) - 1  # all but the empty list
        assert written["desc"].sum() == (want_best >= 0).sum() < written["normal"].sum()
        # without d_best the table is the same
        status, best, got = dev.run(ctx, st, what, before, with_best=False)
        assert status == 0 and best is None
        _same(got, want, "d_best == NULL")


FAULTS = ["row == n_rows", "row == -1", "first offset -1", "descending offset", "last offset beyond n_obs", "obs_kf == n_kfs", "obs_kf == -1",
          "obs_idx == kf.n", "obs_idx == -1", "d_ref == list length", "d_ref == -1", "octave == nlevels", "octave == -1"]


def _faulty_scene(fault):
    """A small scene with ONE fault among good updates.  Returns the scene and the updates the fault makes faulty."""
    s = _clean()
    s = dict(s, **{k: s[k].copy() for k in ("row", "obs_off", "obs_kf", "obs_idx", "ref")}, kf_octave=[o.copy() for o in s["kf_octave"]])
    n_upd = len(s["n_of"])
    q = int(np.nonzero(s["n_of"] == 5)[0][1])  # an update in the middle
    big = int(np.nonzero(s["n_of"] == 70)[0][0])
    o0 = int(s["obs_off"][q])
    hit = [q]
    if fault.startswith("row"):
        s["row"][q] = s["n_rows"] if fault.endswith("n_rows") else -1
    elif fault == "first offset -1":
        s["obs_off"][0], hit = -1, [0]
    elif fault == "descending offset":  # update q - 1 ends before it starts; update q reads a longer, valid list
        assert s["obs_off"][q - 1] > 0
        s["obs_off"][q], hit = s["obs_off"][q - 1] - 1, [q - 1]
    elif fault == "last offset beyond n_obs":
        s["obs_off"][n_upd], hit = len(s["obs_kf"]) + 1, [n_upd - 1]
    elif fault.startswith("obs_kf"):
        s["obs_kf"][o0 + 2] = len(s["kf_n"]) if fault.endswith("n_kfs") else -1
    elif fault == "obs_idx == kf.n":  # in the second block of 64 of a long list
        o, hit = int(s["obs_off"][big]) + 66, [big]
        s["obs_idx"][o] = s["kf_n"][s["obs_kf"][o]]
    elif fault == "obs_idx == -1":
        s["obs_idx"][o0 + 4] = -1
    elif fault.startswith("d_ref"):
        s["ref"][q] = 5 if fault.endswith("length") else -1
    else:  # the octave of the reference keypoint of update q; no other update may use that keypoint as its reference
        kf, idx = int(s["obs_kf"][o0 + s["ref"][q]]), int(s["obs_idx"][o0 + s["ref"][q]])
        s["kf_octave"][kf][idx] = len(SCALE) if fault.endswith("nlevels") else -1
    return s, hit


@pytest.mark.gpu
@pytest.mark.parametrize("fault", FAULTS)
def test_gpu_a_faulty_update_is_skipped_whole_and_reported(gpu, fault):
    """Status INVALID, the faulty update's row untouched with d_best = -1, every other row exact.  The faulty values stay inside the
    test's allocations: one entry beyond either end of a padded list, of the directory (padded with copies of a record), of a
    keyframe's descriptors (inside the common buffer), of the guarded table; the scale table has 16 entries for 8 levels."""
    api, ctx, st, _ = gpu
    import torch
    s, hit = _faulty_scene(fault)
    before = S.fresh_table(s)
    want = {k: v.copy() for k, v in before.items()}
    what = 2 if fault.startswith(("d_ref", "octave")) else 3
    want_best, want_status = M.update_map_points(s, what, want)
    assert want_status == M.ERR_INVALID and all(want_best[h] == -1 for h in hit)
    clean_best, clean_status = M.update_map_points(_clean(), what, S.fresh_table(s))
    assert clean_status == 0 and (what == 2 or all(clean_best[h] >= 0 for h in hit))  # without the fault these updates write their row
    dev = _Device(api, s)
    torch.cuda.synchronize()
    status, best, got = dev.run(ctx, st, what, before)
    assert status == api.ERR_INVALID, fault
    assert np.array_equal(best, want_best), fault
    _same(got, want, fault)
    if not fault.startswith("row"):
        for h in hit:
            r = int(s["row"][h])
            assert all(np.array_equal(got[k][r], before[k][r]) for k in got), "the row of the faulty update was written"


def _clean():
    key = "clean faulty scene"
    if key not in _cache:
        _cache[key] = S.build({1: 3, 3: 4, 5: 4, 40: 2, 70: 2}, n_kfs=96, kp_range=(16, 64), seed=33, extra=("empty",), scale=SCALE, extra_rows=7, permute_rows=True)
    return _cache[key]


@pytest.mark.gpu
def test_gpu_refusals_queue_nothing_and_empty_calls_write_the_status_only(gpu):
    api, ctx, st, device_of = gpu
    s, dev = _scene("null"), device_of("null")
    n_upd = len(s["n_of"])
    status = Guarded.cells(1)
    sp = status.ptr
    good = dict(d_kfs=dev.rec_ptr, n_kfs=len(s["kf_n"]), n_upd=n_upd, d_row=0, n_rows=s["n_rows"], d_obs_off=dev.lists["obs_off"][1],
                d_obs_kf=dev.lists["obs_kf"][1], d_obs_idx=dev.lists["obs_idx"][1], n_obs=len(s["obs_kf"]), d_ref=dev.lists["ref"][1], what=3,
                d_pos=dev.pos[1], d_normal=8, d_max_distance=8, d_min_distance=8, d_pt_desc=8, d_best=0, d_status=sp)
    for kw, message in REFUSED:
        if "d_status" in kw:
            continue
        with pytest.raises(api.OrbfeError) as e:
            ctx.enqueue_update_map_points(**dict(good, **{k: v for k, v in kw.items()}), stream=st.cuda_stream)
        assert e.value.code == api.ERR_INVALID and message in str(e.value), kw
    with pytest.raises(api.OrbfeError):
        ctx.enqueue_update_map_points(**dict(good, n_upd=s["n_rows"] + 1), stream=st.cuda_stream)
    st.synchronize()
    assert status.untouched()
    # n_upd == 0: status 0 and nothing else, whatever the other pointers are
    ctx.enqueue_update_map_points(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0, 0, 0, 0, 0, 0, sp, stream=st.cuda_stream)
    st.synchronize()
    assert int(status.fetch()[0]) == 0


def _chain_scene():
    """The fuse scene, its observation lists as an update scene, the table before and after (the model's), the model's winners."""
    if "chain" in _cache:
        return _cache["chain"]
    name = "retreat"
    f, p = MC.build(name), MC.INPUTS[name][1]["fuse"]
    n = len(f["pos"])
    rng = np.random.default_rng(77)
    T = f["T_cur"].astype(np.float64)
    centre = (-T[:, :3].T @ T[:, 3]).astype(np.float32)
    flip = lambda: f["desc"] ^ np.packbits(rng.random((n, 256)) < 0.04, axis=1, bitorder="little")
    seen = np.full(n, -1, np.int64)
    seen[f["src"][f["src"] >= 0]] = np.nonzero(f["src"] >= 0)[0]
    kf_desc = [f["desc"].copy(), f["d"].copy(), flip(), flip()]
    kf_octave = [f["octave"].astype(np.int32), f["k"]["octave"].astype(np.int32), f["octave"].astype(np.int32), f["octave"].astype(np.int32)]
    obs_off, obs_kf, obs_idx, ref = [0], [], [], []
    for q in range(n):
        entries = [(2, q)] * int(rng.random() < 0.6) + [(0, q)] + [(1, int(seen[q]))] * int(seen[q] >= 0) + [(3, q)] * int(rng.random() < 0.5)
        ref.append(entries.index((0, q)))
        obs_kf += [e[0] for e in entries]; obs_idx += [e[1] for e in entries]
        obs_off.append(len(obs_kf))
    s = dict(kf_n=np.array([len(d) for d in kf_desc], np.int32), kf_bad=np.array([0, 0, 0, 1], np.int32),
             Ow=np.array([[0, 0, 0], centre, [0.3, -0.2, 0.1], [-0.4, 0.1, -0.3]], np.float32), kf_desc=kf_desc, kf_octave=kf_octave,
             nlevels=len(SCALE), scale=SCALE, obs_off=np.asarray(obs_off, np.int32), obs_kf=np.asarray(obs_kf, np.int32),
             obs_idx=np.asarray(obs_idx, np.int32), ref=np.asarray(ref, np.int32), row=None, n_rows=n, n_of=np.diff(obs_off), pos=f["pos"])
    s["kf_desc_int"] = [[M.as_int(d) for d in kd] for kd in kf_desc]
    before = dict(normal=f["normal"], max_d=f["max_d"], min_d=f["min_d"], desc=f["desc"])
    want = {k: v.copy() for k, v in before.items()}
    want_best, want_status = M.update_map_points(s, 3, want)
    assert want_status == 0 and (want["desc"] != before["desc"]).any() and (want["normal"] != before["normal"]).any()
    assert np.allclose(want["max_d"], before["max_d"], rtol=1e-6)  # the scene's own band is |pos| * scale[octave] too
    _cache["chain"] = (f, p, s, before, want, want_best)
    return _cache["chain"]


@pytest.mark.gpu
def test_gpu_fuse_reads_the_rows_the_update_has_just_written_on_the_same_stream(gpu):
    """SearchInNeighbors' closing step and the next target: the rows of a fuse scene (tests/matcher_census.py) are recomputed from
    observation lists -- the keyframe at the origin that created the points (the reference keyframe), the scene's current keyframe
    where it sees the point, two more with flipped bits, one of them bad -- and orbfe_enqueue_fuse follows on the same stream with no
    synchronisation in between.  Its result equals orbfe_enqueue_fuse on a table whose rows the model computed."""
    import torch
    api, ctx, st, _ = gpu
    f, p, s, before, want, want_best = _chain_scene()
    n = len(f["pos"])

    class Table:  # what TF._enqueue wants: the row count and the five column addresses
        def __init__(self, pos_ptr, cols):
            self.n, self.p = n, [pos_ptr] + [cols[k].ptr for k in ("normal", "max_d", "min_d", "desc")]

        def ptrs(self):
            return self.p

    kf, d_valid = TF._kf_of(api, ctx, st, f, f["ur"]), upload(f["valid"], pad=TF.PAD)[0]
    dev = _Device(api, s)
    model_cols = {k: Guarded(want[k]) for k in want}
    out_ref = TF._Out(n)
    torch.cuda.synchronize()
    TF._enqueue(ctx, False, kf.rec, f["T_cur"], Table(dev.pos[1], model_cols), d_valid, p[0], out_ref, st)
    st.synchronize()
    ref_best, ref_count, ref_status = out_ref.fetch()
    stale = TF._Out(n)
    stale_cols = {k: Guarded(before[k]) for k in before}
    torch.cuda.synchronize()
    TF._enqueue(ctx, False, kf.rec, f["T_cur"], Table(dev.pos[1], stale_cols), d_valid, p[0], stale, st)
    st.synchronize()
    assert ref_status == 0 and ref_count > 100 and not np.array_equal(stale.fetch()[0], ref_best)  # the rewritten rows decide something
    # the chain: update, then fuse, one synchronise
    cols = {k: Guarded(before[k]) for k in before}
    out = TF._Out(n)
    best, status = Guarded.cells(n), Guarded.cells(1)
    torch.cuda.synchronize()
    ctx.enqueue_update_map_points(dev.rec_ptr, 4, n, 0, n, dev.lists["obs_off"][1], dev.lists["obs_kf"][1], dev.lists["obs_idx"][1], len(s["obs_kf"]),
                                  dev.lists["ref"][1], 3, dev.pos[1], cols["normal"].ptr, cols["max_d"].ptr, cols["min_d"].ptr, cols["desc"].ptr,
                                  best.ptr, status.ptr, stream=st.cuda_stream)
    TF._enqueue(ctx, False, kf.rec, f["T_cur"], Table(dev.pos[1], cols), d_valid, p[0], out, st)
    st.synchronize()
    assert int(status.fetch()[0]) == 0 and np.array_equal(best.fetch(), want_best)
    _same({k: c.fetch() for k, c in cols.items()}, want, "chain")
    TF._check(out, ref_best, ref_count, "fuse behind the update")
