"""MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth off the GPU: hand-written known answers for the literal
model (tests/map_point_model.py), the census of what the committed scenes decide, and the C++ host mirror
(orbslam2_amd/host/MapPointUpdate.h, driven by tests/map_point_mirror/mirror_main.cpp) equal to the model bit for bit -- built plain
and as a stand-alone AddressSanitizer + UBSan program."""
import numpy as np
import pytest

from tests import host_forms as H
from tests import map_point_model as M
from tests import map_point_scenes as S


def _d(*bits):
    """A descriptor with exactly these bits set: the distance of two of them is the size of the symmetric difference."""
    return sum(1 << b for b in bits)


def _winner(descs, bad=None):
    return M.compute_distinctive_descriptors(descs, bad or [0] * len(descs))[0]


# ------------------------------------------------------------------ known answers
def test_descriptor_known_answers():
    A, B, C = _d(), _d(0), _d(*range(1, 11))             # d(A,B) = 1, d(A,C) = 10, d(B,C) = 11
    assert _winner([C]) == 0                              # N = 1
    assert _winner([C, A]) == 0 and _winner([A, C]) == 0  # N = 2: both medians are the own 0, entry 0 wins the tie
    assert M.compute_distinctive_descriptors([C, A], [0, 0])[1:] == (0, 2)
    # N = 3, d01 smallest: rows (0, 1, 10), (0, 1, 11), (0, 10, 11), k = 1: entries 0 and 1 tie at 1, entry 0 wins
    assert M.compute_distinctive_descriptors([A, B, C], [0, 0, 0]) == (0, 1, 2)
    assert _winner([B, A, C]) == 0 and _winner([C, A, B]) == 1 and _winner([C, B, A]) == 1
    # the median index is (int)(0.5 * (N - 1)): with N = 4 it is the SECOND smallest of a row, its own 0 included
    D = _d(*range(1, 11), 20)                             # d(C,D) = 1, d(A,D) = 11, d(B,D) = 12
    assert M.compute_distinctive_descriptors([A, C, D, B], [0] * 4) == (0, 1, 4)
    assert M.compute_distinctive_descriptors([A, C, D, _d(*range(30, 90))], [0] * 4) == (1, 1, 2)
    # empty list, all-bad list
    assert _winner([]) == -1 and _winner([A, B, C], [1, 1, 1]) == -1


def test_dropping_a_bad_keyframe_changes_the_winner_and_the_position_is_the_lists():
    A, B, C = _d(), _d(0), _d(*range(1, 11))
    assert _winner([C, A, B]) == 1                        # medians 10, 1, 1
    assert _winner([C, A, B], [0, 1, 0]) == 0             # G = (C, B): a tie at 0, C wins
    P, Q, R = _d(*range(100, 105)), _d(), _d(0)           # medians 5, 1, 1: Q is entry 1 of G and entry 2 of the list
    assert _winner([A, P, Q, R], [1, 0, 0, 0]) == 2
    assert _winner([P, A, Q, A, R], [0, 1, 0, 1, 0]) == 2


def test_normal_known_answer_differs_from_the_divide_variant():
    """n = 3: multiplying by (float)(1.0 / 3) and by (float)(1.0 / norm) is not dividing; the expected bits were worked out once with
    the steps of the contract and are written out here."""
    pos = [2.5, -3.5, -2.5]
    centres = [[-1.0, -1.25, 1.25], [1.5, 0.25, -2.0], [-1.75, -0.75, -0.25]]
    normal, mx, mn = M.update_normal_and_depth(pos, centres, 1, 2, S.SCALE, 8)
    bits = lambda v: [int(np.float32(x).view(np.uint32)) for x in v]
    assert bits(normal) == [0x3F0C9862, 0xBF1E6A48, 0xBECD6254]
    assert bits([mx, mn]) == [0x40B45108, 0x3FC94AC6]
    other = M.update_normal_and_depth(pos, centres, 1, 2, S.SCALE, 8, divide=True)
    assert bits(other[0]) == [0x3F0C9861, 0xBF1E6A47, 0xBECD6254] and bits(other[1:]) == bits([mx, mn])
    # the depth band by hand: |pos - centre 1| = sqrt(1 + 14.0625 + 0.25), times 1.2^2, over 1.2^7
    d = np.float32(np.sqrt(np.float64(15.3125)))
    assert mx == d * S.SCALE[2] and mn == mx / S.SCALE[7]


# ------------------------------------------------------------------ census of the committed scenes
@pytest.fixture(scope="module")
def census():
    s = S.census_scene()
    table = S.fresh_table(s)
    before = {k: v.copy() for k, v in table.items()}
    best, status = M.update_map_points(s, 3, table)
    return s, before, table, best, status


def test_census_scenes_decide_what_the_kernel_can_get_wrong(census):
    s, before, table, best, status = census
    assert status == 0
    for N in S.CENSUS_NS:
        ties = not_first = bad_matters = 0
        for q in np.nonzero(s["n_of"] == N)[0]:
            obs = [(s["obs_kf"][o], s["obs_idx"][o]) for o in range(s["obs_off"][q], s["obs_off"][q + 1])]
            descs = [s["kf_desc_int"][kf][idx] for kf, idx in obs]
            w, _, sharing = M.compute_distinctive_descriptors(descs, [int(s["kf_bad"][kf]) for kf, _ in obs])
            assert w == best[q]
            ties += sharing > 1
            not_first += w > 0
            if N >= 3 and not bad_matters and any(s["kf_bad"][kf] for kf, _ in obs):
                bad_matters += M.compute_distinctive_descriptors(descs, [0] * len(descs))[0] != w
        assert N < 2 or ties > 0, N
        assert N < 3 or (not_first > 0 and bad_matters > 0), N
    # the empty list and the all-bad list leave the descriptor row alone; the all-bad list still gets its normal (:350 does not test isBad)
    empty = int(np.nonzero(s["n_of"] == 0)[0][0])
    all_bad = [q for q in np.nonzero(s["n_of"] == 3)[0] if all(s["kf_bad"][s["obs_kf"][o]] for o in range(s["obs_off"][q], s["obs_off"][q + 1]))]
    assert best[empty] == -1 and all(np.array_equal(table[k][empty], before[k][empty]) for k in table)
    assert len(all_bad) >= 1 and all(best[q] == -1 for q in all_bad)
    q = all_bad[0]
    assert np.array_equal(table["desc"][q], before["desc"][q]) and not np.array_equal(table["normal"][q], before["normal"][q])
    # no slot of a keyframe is shared in this scene: every observation has a descriptor of its own point
    pairs = set(zip(s["obs_kf"].tolist(), s["obs_idx"].tolist()))
    assert len(pairs) == len(s["obs_kf"])


# ------------------------------------------------------------------ the C++ mirror
def _run(exe, s, table, what, tmp_path):
    scene, out = str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")
    S.write_scene_file(s, table, what, scene)
    H.run(exe, scene, out)
    return S.read_result_file(s, out)


def _same(got, want, what):
    for k in want:
        a, b = np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8)
        assert np.array_equal(a, b), "%s: column %s differs in rows %s" % (what, k, np.nonzero((a != b).reshape(len(b), -1).any(axis=1))[0][:8].tolist())


@pytest.mark.parametrize("build", H.BUILDS)
def test_cpp_mirror_equals_the_model_bit_for_bit(census, tmp_path, build):
    s, before, want, best, status = census
    exe = H.build(tmp_path, "map_point_mirror", build)
    got_status, got_best, got = _run(exe, s, before, 3, tmp_path)
    assert got_status == status == 0 and np.array_equal(got_best, best)
    _same(got, want, "census scene")
    # one column set at a time through a permuted row list into a larger table, with faulty updates among good ones
    t = S.build({1: 3, 2: 3, 5: 4, 65: 2, 70: 1}, seed=4, extra=("empty", "all_bad"), extra_rows=9, permute_rows=True)
    t["obs_idx"][t["obs_off"][3]] = -1
    t["ref"][6] = t["obs_off"][7] - t["obs_off"][6]
    for what in (1, 2, 3):
        table = S.fresh_table(t)
        mine = {k: v.copy() for k, v in table.items()}
        want_best, want_status = M.update_map_points(t, what, mine)
        got_status, got_best, got = _run(exe, t, table, what, tmp_path)
        assert got_status == want_status == M.ERR_INVALID and np.array_equal(got_best, want_best)
        _same(got, mine, "what = %d" % what)
        if what == 1:
            assert np.array_equal(mine["normal"], table["normal"]) and np.array_equal(mine["max_d"], table["max_d"])
        if what == 2:
            assert np.array_equal(mine["desc"], table["desc"])


def test_the_mirror_header_includes_nothing_but_the_c_abi_header():
    assert H.project_includes(H.header("MapPointUpdate.h")) == H.ABI_AND_CVMAT
