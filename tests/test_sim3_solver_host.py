"""orbslam2_amd/host/Sim3Solver.h against the model (tests/sim3_solver_model.py) bit for bit, on the scenes of tests/sim3_solver_scenes.py:
the iteration table, the filter's rows, the sets, every hypothesis record, the inlier bits and the events; and ORB_SLAM2::Sim3Solver's
iterate / find against the literal transcription of src/Sim3Solver.cc:141-208 with nIterations 1, 5 and 300, including count rows whose
event falls on the last iteration.  The comparison is made by a stand-alone driver with its own main
(tests/sim3_solver_mirror/mirror_main.cpp), built through tests/host_forms.py plain and as an AddressSanitizer + UBSan program; nothing
is loaded into Python."""
import numpy as np
import pytest

from tests import host_forms as HF
from tests import sim3_solver_model as M
from tests import sim3_solver_scenes as S
from tests.test_sim3_solver_model import LAST_ITERATION_COUNTS, literal_walk

SCENES = ["outliers", "clean", "fix_scale", "n65", "invalid_slots", "below_min", "at_min", "gate", "coincident", "cand_b"]
REPLAYS = [(40, c, 20, step) for c in LAST_ITERATION_COUNTS for step in (1, 5, 300)] + [(10, [30, 30], 20, 5)]


def test_header_includes_only_the_abi_and_cvmat():
    assert HF.project_includes(HF.header("Sim3Solver.h")) == HF.ABI_AND_CVMAT
    text = open(HF.header("Sim3Solver.h")).read()
    assert not [ln for ln in text.splitlines() if ln.startswith("#include") and "opencv" in ln.lower()]


def _problem():
    i32 = lambda *v: np.array(v, np.int32).tobytes()
    out = [i32(len(SCENES))]
    for name in SCENES:
        s = S.scene(name)
        out += [i32(len(s["keys1"]), len(s["keys2"]), len(s["pairs"]), s["max_pairs"], s["max_its"], s["min_inliers"], s["fix_scale"], len(s["sigma2"])),
                np.float64(s["prob"]).tobytes(), np.array(s["cam"], np.float32).tobytes(), s["sigma2"].tobytes(), s["T1w"].tobytes(), s["T2w"].tobytes()]
        for k in ("1", "2"):
            out += [s["keys" + k].tobytes(), np.ascontiguousarray(s["pos" + k], np.float32).tobytes(), s["valid" + k].astype(np.int32).tobytes()]
        out += [np.ascontiguousarray(s["pairs"], np.int32).tobytes(), np.ascontiguousarray(s["draws"], np.uint32).tobytes()]
    out.append(i32(len(REPLAYS)))
    for N, counts, mn, step in REPLAYS:
        out += [i32(N, len(counts), mn, step, len(counts)), i32(*counts)]
    return b"".join(out)


class _Reader:
    def __init__(self, data):
        self.d, self.at = data, 0

    def take(self, dtype, n):
        a = np.frombuffer(self.d, dtype, n, self.at)
        self.at += a.nbytes
        return a


def _replay_log(r):
    calls = int(r.take(np.int32, 1)[0])
    return r.take(np.int32, 5 * calls).reshape(calls, 5)


@pytest.mark.parametrize("build", HF.BUILDS)
def test_host_form_equals_the_model_bit_for_bit(tmp_path, build):
    exe = HF.build(tmp_path, "sim3_solver_mirror", build)
    (tmp_path / "problem.bin").write_bytes(_problem())
    HF.run(exe, str(tmp_path / "problem.bin"), str(tmp_path / "out.bin"))
    r = _Reader((tmp_path / "out.bin").read_bytes())
    for name in SCENES:
        s, m = S.scene(name), S.model(name)
        mp, mi, words = s["max_pairs"], s["max_its"], (s["max_pairs"] + 31) // 32
        status, n_corr, n_its, n_events = r.take(np.int32, 4)
        assert (status, n_corr, n_its, n_events) == (m["status"], m["n_corr"], m["n_its"], m["n_events"]), name
        assert np.array_equal(r.take(np.int32, mp + 1), s["its_for_n"]), name
        assert np.array_equal(r.take(np.int32, 2 * mp).reshape(mp, 2), m["corr"]), name
        assert np.array_equal(r.take(np.int32, 3 * mi).reshape(mi, 3), m["sets"]), name
        assert np.array_equal(r.take(np.int32, mi), m["events"]), name
        hyp = r.take(M.HYP_DTYPE, mi)
        assert np.array_equal(hyp["n_inliers"], m["hyp"]["n_inliers"]), name
        assert hyp.tobytes() == m["hyp"].tobytes(), (name, np.nonzero(HF.bits(hyp) != HF.bits(m["hyp"]))[0][:8] // 64)
        assert np.array_equal(r.take(np.uint32, mi * words).reshape(mi, words), m["bits"]), name
        counts = m["hyp"]["n_inliers"][:n_its]
        for step in (1, 5, 300):
            log = _replay_log(r)
            want = literal_walk(n_corr, counts, s["min_inliers"], step)
            assert [(k, bool(b), n, it) for k, b, n, _, it in log.tolist()] == want, (name, step)
            for k, _, n, slots, _ in log.tolist():                     # vbInliers is indexed by KF1's slots (mvnIndices1)
                assert slots == (n if k >= 0 else 0), (name, step)
    for N, counts, mn, step in REPLAYS:
        log = _replay_log(r)
        assert [(k, bool(b), n, it) for k, b, n, _, it in log.tolist()] == literal_walk(N, np.array(counts, np.int32), mn, step), (counts, step)
    assert r.at == len(r.d)
