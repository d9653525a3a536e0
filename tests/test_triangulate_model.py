"""The triangulation stage of LocalMapping::CreateNewMapPoints off the GPU: hand-made known answers for the literal model
(tests/triangulate_model.py; those of its null vector are in tests/test_cvmat_model.py), the census of what the committed scenes decide (tests/triangulate_scenes.py), the model against a float64
restatement with numpy.linalg.svd, and the C++ host form (orbslam2_amd/host/Triangulate.h, driven by
tests/triangulate_mirror/mirror_main.cpp) equal to the model bit for bit -- built plain and as a stand-alone AddressSanitizer + UBSan
program."""
import collections
import ctypes as C
import os

import numpy as np
import pytest

from tests import host_forms as H
from tests import triangulate_model as M
from tests import triangulate_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "orbfe_enqueue_triangulate_pairs"
F32 = np.float32
# The largest relative deviation of x3D, model against the float64 restatement, measured over the generic scenes on the CPU is 1.33e-6
# (scene "wide"; "narrow" 1.5e-7).  The bound is 4 times that: headroom for conditioning across seeds, not for the kernel or the C++
# form, which equal the model bit for bit.
MEASURED_MAX_REL = 1.33e-6
X3D_REL_TOL = 4 * MEASURED_MAX_REL
MARGIN = 1e-4            # codes are compared where every gate the float64 form evaluated is decided by more than this, relatively
MAX_LEFT_OUT = 0.02      # ... and those left out are at most this share of a scene


# ------------------------------------------------------------------ known answers: one pair per code
def _two_cameras(n=4):
    T1 = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    T2 = np.concatenate([np.eye(3), np.array([[-1.0], [0.0], [0.0]])], axis=1)   # 1 m to the right of camera 1
    return S.keyframe(T1, n), S.keyframe(T2, n), T1, T2


def _see(kf, T, i, Pw, octave=0):
    pc = T[:, :3] @ np.asarray(Pw, float) + T[:, 3]
    kf["keys_un"]["x"][i] = S.FX * pc[0] / pc[2] + S.CX; kf["keys_un"]["y"][i] = S.FY * pc[1] / pc[2] + S.CY
    kf["keys_un"]["octave"][i] = octave
    return pc


def _code(kf1, kf2, i1=0, i2=0):
    sf, s2 = S.levels()
    with np.errstate(all="ignore"):
        return M.pair(kf1, kf2, i1, i2, S.MBF, S.RATIO_FACTOR, sf, s2)


def test_one_hand_made_pair_for_each_of_the_twelve_codes():
    P = [0.5, 0.25, 5.0]
    # 0: a true correspondence, 1 m baseline, 5 m away
    kf1, kf2, T1, T2 = _two_cameras()
    _see(kf1, T1, 0, P); _see(kf2, T2, 0, P)
    c, X, info = _code(kf1, kf2)
    assert c == M.TRIANGULATED and np.allclose(X, P, rtol=1e-5) and info["sweeps"] >= 1
    # 10: the same pair seen four octaves apart (1.2^4 > 1.5 * 1.2)
    kf2["keys_un"]["octave"][0] = 4
    assert _code(kf1, kf2)[0] == M.SCALE
    kf2["keys_un"]["octave"][0] = 0
    # 9: GetCameraCenter() of KF2 is handed over; at the triangulated point the distance is zero
    kf2["Ow"] = np.array(X, F32)
    assert _code(kf1, kf2)[0] == M.ZERO_DIST
    # 7 / 8: the point moved 12 px in one image only is triangulated between the rays, 6 px from either keypoint; KF1's test comes first.
    # A KF1 keypoint at octave 7 (5.991 * sigma2 = 76.9 > 36) passes, and KF2 at octave 4 (25.8) fails
    kf1, kf2, T1, T2 = _two_cameras()
    _see(kf1, T1, 0, P); _see(kf2, T2, 0, P)
    kf2["keys_un"]["y"][0] += 12
    assert _code(kf1, kf2)[0] == M.REPROJ1
    kf1["keys_un"]["octave"][0] = 7; kf2["keys_un"]["octave"][0] = 4
    assert _code(kf1, kf2)[0] == M.REPROJ2
    # 5: the rays diverge (the images swapped): the intersection lies behind both cameras
    kf1, kf2, T1, T2 = _two_cameras()
    _see(kf1, T2, 0, P); _see(kf2, T1, 0, P)
    assert _code(kf1, kf2)[0] == M.Z1
    # 6: KF2 stands 8 m ahead of KF1; KF1's stereo point 5 m away is unprojected (parallel rays) and lies behind KF2
    kf1, kf2, T1, _ = _two_cameras()
    T2 = np.concatenate([np.eye(3), np.array([[0.0], [0.0], [-8.0]])], axis=1)
    kf2 = S.keyframe(T2, 4)
    pc = _see(kf1, T1, 0, P)
    S.set_stereo(kf1, 0, F32(kf1["keys_un"]["x"][0] - float(S.MBF) / pc[2]))
    kf2["keys_un"]["x"][0], kf2["keys_un"]["y"][0] = kf1["keys_un"]["x"][0], kf1["keys_un"]["y"][0]
    assert _code(kf1, kf2)[0] == M.Z2
    # 1 / 2 / 3: two cameras 1 cm apart; stereo in KF1 unprojects KF1, stereo in KF2 only unprojects KF2, stereo in both uses KF1's
    # cosine alone (`else if (bStereo2)`), no stereo is low parallax
    T1 = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    T2 = np.concatenate([np.eye(3), np.array([[-0.01], [0.0], [0.0]])], axis=1)
    for stereo1, stereo2, want in ((1, 0, M.STEREO1), (0, 1, M.STEREO2), (1, 1, M.STEREO1), (0, 0, M.LOW_PARALLAX)):
        kf1, kf2 = S.keyframe(T1, 4), S.keyframe(T2, 4)
        for kf, T, st in ((kf1, T1, stereo1), (kf2, T2, stereo2)):
            pc = _see(kf, T, 0, P)
            if st:
                S.set_stereo(kf, 0, F32(kf["keys_un"]["x"][0] - float(S.MBF) / pc[2]))
        c, X, _ = _code(kf1, kf2)
        assert c == want, (stereo1, stereo2, c)
        if want != M.LOW_PARALLAX:
            assert np.allclose(X, P, rtol=1e-4)
    # ... with both stereo KF2's cosine is NOT consulted: were it, the smaller one below would make this UnprojectStereo(KF2)
    kf1, kf2 = S.keyframe(T1, 4), S.keyframe(T2, 4)
    for kf, T in ((kf1, T1), (kf2, T2)):
        pc = _see(kf, T, 0, P)
        S.set_stereo(kf, 0, F32(kf["keys_un"]["x"][0] - float(S.MBF) / pc[2]))
    kf2["cos"][0] = F32(0.5)
    assert _code(kf1, kf2)[0] == M.STEREO1
    kf1["ur"][0] = -1.0
    assert _code(kf1, kf2)[0] == M.STEREO2
    # 2 reads mvKeys, not mvKeysUn
    kf1, kf2 = S.keyframe(T1, 4), S.keyframe(T2, 4)
    _see(kf1, T1, 0, P); pc = _see(kf2, T2, 0, P)
    S.set_stereo(kf2, 0, F32(kf2["keys_un"]["x"][0] - float(S.MBF) / pc[2]))
    same = _code(kf1, kf2)[1]
    kf2["keys"] = kf2["keys_un"].copy(); kf2["keys"]["x"][0] += 5
    moved = _code(kf1, kf2)
    assert moved[0] in (M.STEREO2, M.REPROJ1, M.REPROJ2) and (moved[1] is None or moved[1][0] != same[0])
    # 4: the degenerate scene's skew rays; 11: every device-checked fault
    d = S.degenerate()
    assert _code(d["kf1"], d["kf2"], 0, 19)[0] == M.W_ZERO
    kf1, kf2, T1, T2 = _two_cameras()
    _see(kf1, T1, 0, P); _see(kf2, T2, 0, P)
    assert [_code(kf1, kf2, a, b)[0] for a, b in ((4, 0), (0, 4), (-1, 0), (0, -1))] == [M.FAULTY] * 4
    kf1["keys_un"]["octave"][0] = S.NLEVELS
    assert _code(kf1, kf2)[0] == M.FAULTY
    kf1["keys_un"]["octave"][0] = 0; kf2["keys_un"]["octave"][0] = -1
    assert _code(kf1, kf2)[0] == M.FAULTY
    kf2["keys_un"]["octave"][0] = 0; kf2["ur"][0] = 100.0; kf2["depth"][0] = 0.0
    assert _code(kf1, kf2)[0] == M.FAULTY
    kf2["ur"][0] = -1.0
    assert _code(kf1, kf2)[0] == M.TRIANGULATED


# ------------------------------------------------------------------ census of the committed scenes
def test_census_scenes_reach_every_code_both_stereo_sources_and_both_rotation_branches():
    total, sweeps = collections.Counter(), collections.Counter()
    beta = collections.Counter()
    for name in S.SCENES:
        code, _, infos, res = S.census(name)
        p = S.scene(name)
        assert res["status"] == 0 and res["nnew"] == int((code <= M.CREATED_MAX).sum()), name
        total.update(code.tolist())
        sweeps.update(i["sweeps"] for i in infos if i)
        beta.update(i["first_beta_negative"] for i in infos if i and i["rotations"])
        if name in ("wide", "narrow"):               # mixed stereo and monocular keypoints on both sides of the pairs
            for kf, col in ((p["kf1"], 0), (p["kf2"], 1)):
                st = kf["ur"][p["pairs"].reshape(-1, 2)[:p["npairs"], col]] >= 0
                assert 0.2 < st.mean() < 0.8, name
    print("codes", sorted(total.items()), "sweeps", sorted(sweeps.items()), "first beta < 0", dict(beta))
    for c in range(M.FAULTY):
        assert total[c] >= 5, (c, total[c])
    assert total[M.FAULTY] == 0
    assert total[M.STEREO1] >= 5 and total[M.STEREO2] >= 5
    assert beta[True] >= 50 and beta[False] >= 50
    assert min(sweeps) >= 2 and sweeps[M.MAX_SWEEPS] >= 5          # exact data never converges: the sweep cap is reached
    assert sum(v for k, v in sweeps.items() if k <= 4) > 0.98 * sum(sweeps.values()) - sweeps[M.MAX_SWEEPS]
    swaps = collections.Counter(i["swaps"] for i in S.census("degenerate")[2] if i)
    assert swaps[1] >= 1 and swaps[2] >= 1                          # the selection sort moves rows


# ------------------------------------------------------------------ the model against float64
@pytest.mark.parametrize("name", S.GENERIC)
def test_model_equals_the_float64_restatement_where_the_gates_are_decided(name):
    p = S.scene(name)
    code, x3d, _, _ = S.census(name)
    left_out, worst = 0, 0.0
    with np.errstate(all="ignore"):
        for q in range(p["npairs"]):
            i1, i2 = int(p["pairs"][2 * q]), int(p["pairs"][2 * q + 1])
            c, X, margin = M.pair_f64(p["kf1"], p["kf2"], i1, i2, p["mbf"], p["ratio"], p["sf"], p["s2"])
            if not margin > MARGIN:
                left_out += 1
                continue
            assert c == code[q], (name, q, c, int(code[q]), margin)
            if c <= M.CREATED_MAX:
                worst = max(worst, float(np.linalg.norm(x3d[q].astype(np.float64) - X) / np.linalg.norm(X)))
    print(name, "left out", left_out, "of", p["npairs"], "largest relative deviation of x3D", worst)
    assert left_out <= MAX_LEFT_OUT * p["npairs"], (name, left_out)
    assert worst <= X3D_REL_TOL, (name, worst)


# ------------------------------------------------------------------ the call: order, table, capacity, patch
def test_the_call_appends_in_pair_order_and_refuses_a_full_table_whole():
    p0 = S.scene("narrow")
    code = S.census("narrow")[0]
    created = np.nonzero(code <= M.CREATED_MAX)[0]
    nnew = len(created)
    p = S.fresh(p0)
    out = S.Outputs(p, n_rows=nnew + 7, rows_used=7)
    res = S.run_model(p, out)
    assert res == dict(status=0, nnew=nnew, rows_used=7 + nnew, infos=res["infos"])
    pr = p["pairs"].reshape(-1, 2)
    assert np.array_equal(out.new[:3 * nnew].reshape(-1, 3), np.column_stack([pr[created], 7 + np.arange(nnew)]))
    assert (out.new[3 * nnew:] == S.Outputs.SENT_I32).all() and (out.pos[:7] == F32(-555.0)).all()
    assert np.array_equal(out.pos[7:], out.x3d[created])
    assert p["kf1"]["mp"][pr[created, 0]].all() and p["kf2"]["mp"][pr[created, 1]].all()
    changed1 = np.nonzero(p["kf1"]["mp"] != p0["kf1"]["mp"])[0]
    assert len(changed1) > 20 and set(changed1) <= set(pr[created, 0])
    # one row fewer: everything but table, counter and has_mp
    p = S.fresh(p0)
    small = S.Outputs(p, n_rows=nnew + 6, rows_used=7)
    res = S.run_model(p, small)
    assert (res["status"], res["nnew"], res["rows_used"]) == (M.ERR_CAPACITY, nnew, 7)
    assert np.array_equal(small.code, out.code) and np.array_equal(small.x3d, out.x3d) and (small.pos == F32(-555.0)).all()
    assert np.array_equal(small.new[:3 * nnew].reshape(-1, 3), np.column_stack([pr[created], np.full(nnew, -1)]))
    assert np.array_equal(p["kf1"]["mp"], p0["kf1"]["mp"]) and np.array_equal(p["kf2"]["mp"], p0["kf2"]["mp"])
    # a count outside [0, max_pairs] writes nothing at all
    for bad in (-1, p0["max_pairs"] + 1):
        p = S.fresh(p0, npairs=bad)
        o = S.Outputs(p, n_rows=4)
        res = S.run_model(p, o)
        assert (res["status"], res["nnew"]) == (M.ERR_INVALID, None) and (o.code == S.Outputs.SENT_U8).all() and (o.new == S.Outputs.SENT_I32).all()


# ------------------------------------------------------------------ the C++ host form
def _run(exe, p, out, patch, tmp_path):
    problem, result = str(tmp_path / "problem.bin"), str(tmp_path / "out.bin")
    S.write_problem_file(p, out, patch, problem)
    H.run(exe, problem, result)
    return S.read_result_file(p, out, result)


def mirror_cases():
    """(what, problem, n_rows or None, rows_used, patch): every scene with table and patch, then the variants and the faults."""
    cases = [(name, S.scene(name), 900, 11, 1) for name in S.SCENES]
    narrow = S.scene("narrow")
    nnew = int((S.census("narrow")[0] <= M.CREATED_MAX).sum())
    cases += [("no table", narrow, None, 0, 1), ("no patch", narrow, 900, 0, 0), ("mvKeys differ", S.with_distorted_keys(narrow), 900, 3, 1),
              ("table exactly full", narrow, nnew + 5, 5, 1), ("table one row short", narrow, nnew + 4, 5, 1), ("negative counter", narrow, 900, -1, 1),
              ("count -1", S.fresh(narrow, npairs=-1), 900, 0, 1), ("count max + 1", S.fresh(narrow, npairs=narrow["max_pairs"] + 1), 900, 0, 1),
              ("count 0", S.fresh(narrow, npairs=0), 900, 4, 1), ("count below the bound", S.fresh(narrow, npairs=131), 900, 4, 1),
              ("max_pairs 0", S.problem(narrow["kf1"], narrow["kf2"], []), 900, 4, 1)]
    faults = S.fresh(narrow)
    pr = faults["pairs"].reshape(-1, 2)
    pr[3, 0] = faults["kf1"]["n"]; pr[40, 1] = -1
    faults["kf1"]["keys_un"]["octave"][pr[77, 0]] = S.NLEVELS
    i2 = pr[100, 1]
    faults["kf2"]["ur"][i2] = 50.0; faults["kf2"]["depth"][i2] = 0.0
    cases.append(("four faulty pairs", faults, 900, 0, 1))
    return cases


@pytest.mark.parametrize("build", H.BUILDS)
def test_cpp_host_form_equals_the_model_bit_for_bit(tmp_path, build):
    exe = H.build(tmp_path, "triangulate_mirror", build)
    for what, p0, n_rows, rows_used, patch in mirror_cases():
        mine, theirs = S.fresh(p0), S.fresh(p0)
        want = S.Outputs(mine, n_rows, rows_used)
        res = S.run_model(mine, want, patch)
        got_res, got, mp1, mp2 = _run(exe, theirs, S.Outputs(theirs, n_rows, rows_used), patch, tmp_path)
        assert got_res == {k: res[k] for k in ("status", "nnew", "rows_used")}, (what, got_res, res["status"], res["nnew"], res["rows_used"])
        for k in ("code", "x3d", "new") + (("pos",) if n_rows is not None else ()):
            a, b = H.bits(getattr(got, k)), H.bits(getattr(want, k))
            assert np.array_equal(a, b), "%s: %s differs at bytes %s" % (what, k, np.nonzero(a != b)[0][:8].tolist())
        assert np.array_equal(mp1, mine["kf1"]["mp"]) and np.array_equal(mp2, mine["kf2"]["mp"]), what
        if what == "four faulty pairs":
            assert res["status"] == M.ERR_INVALID and sorted(np.nonzero(want.code == M.FAULTY)[0].tolist()) == [3, 40, 77, 100]
        if what == "table one row short":
            assert res["status"] == M.ERR_CAPACITY
        if what == "negative counter":
            assert res["status"] == M.ERR_INVALID and res["rows_used"] == -1


def test_the_host_header_includes_nothing_but_the_c_abi_header():
    assert H.project_includes(H.header("Triangulate.h")) == H.ABI_AND_CVMAT


# ------------------------------------------------------------------ exports
def test_the_library_exports_the_call_and_the_keyframe_record_has_the_documented_size():
    from orbslam2_amd import api
    L = api.load()
    assert NAME in api.EXPORTS
    fn = getattr(L, NAME)  # AttributeError: the symbol is not exported
    args = [0 if t is C.c_int else 0.0 if t is C.c_float else None for t in fn.argtypes]
    assert fn(*args) == api.ERR_INVALID
    assert callable(api.Context.enqueue_triangulate_pairs)
    assert C.sizeof(api.NewpointKeyframe) == 136
    assert [n for n, _ in api.NewpointKeyframe._fields_] == ["keys_un", "keys", "u_right", "depth", "cos_stereo", "has_mp", "Tcw", "Ow", "fx", "fy", "cx", "cy",
                                                            "invfx", "invfy", "n"]
    assert api.NewpointKeyframe.Tcw.offset == 48 and api.NewpointKeyframe.n.offset == 132
    header = open(os.path.join(ROOT, "include", "orbfe.h")).read()
    assert "} orbfe_newpoint_keyframe;" in header and "136 bytes" in header
