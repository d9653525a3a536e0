"""orbslam2_amd/host/PnPsolver.h against the model (tests/pnp_solver_model.py) bit for bit, on the scenes of tests/pnp_solver_scenes.py:
the iteration table, the filter's rows, the sets, every hypothesis and refinement record, both inlier bit rows, the events and the
exhausted exit; and ORB_SLAM2::PnPsolver's iterate against the literal transcription of src/PnPsolver.cc:166-259 with nIterations 1, 5
and 300, including hand-written rows: a success on the last iteration, exhaustion with and without a best hypothesis, N below and at
mRansacMinInliers, and calls made after a success.  The comparison is made by a stand-alone driver with its own main
(tests/pnp_solver_mirror/mirror_main.cpp), built through tests/host_forms.py plain and as an AddressSanitizer + UBSan program; nothing
is loaded into Python."""
import numpy as np
import pytest

from tests import host_forms as HF
from tests import pnp_solver_model as M
from tests import pnp_solver_scenes as S
from tests.test_pnp_solver_model import REPLAYS, literal_walk

SCENES = list(S.SPECS)             # every scene, the 300-iteration ones and the 1025-correspondence one included


def test_header_includes_only_the_abi_and_cvmat():
    assert HF.project_includes(HF.header("PnPsolver.h")) == HF.ABI_AND_CVMAT
    text = open(HF.header("PnPsolver.h")).read()
    assert not [ln for ln in text.splitlines() if ln.startswith("#include") and "opencv" in ln.lower()]


def _problem():
    i32 = lambda *v: np.array(v, np.int32).tobytes()
    out = [i32(len(SCENES))]
    for name in SCENES:
        s = S.scene(name)
        out += [i32(len(s["keys"]), len(s["valid"]), s["capacity"], s["max_its"], s["min_inliers"], s["n_iterations"], len(s["sigma2"]), S.MAX_ITS),
                np.array([s["epsilon"], s["th2"]], np.float32).tobytes(), np.float64(s["prob"]).tobytes(), np.array(s["cam"], np.float32).tobytes(),
                s["sigma2"].tobytes(), s["keys"].tobytes(), s["f_match"].tobytes(), np.ascontiguousarray(s["pos"], np.float32).tobytes(),
                s["valid"].astype(np.int32).tobytes(), np.ascontiguousarray(s["draws"], np.uint32).tobytes()]
    out.append(i32(len(REPLAYS)))
    for N, its, mn, step, counts, ok in REPLAYS:
        out += [i32(N, its, mn, step, len(counts)), i32(*counts), i32(*ok)]
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
    return [tuple(row) for row in r.take(np.int32, 6 * calls).reshape(calls, 6).tolist()]


def _same_records(got, ref, name, what):
    bad = np.nonzero((got.view(np.uint32).reshape(-1, 16) != ref.view(np.uint32).reshape(-1, 16)).any(1))[0]
    assert bad.size == 0, (name, what, bad[:8].tolist(), got[bad[:1]], ref[bad[:1]])


@pytest.mark.parametrize("build", HF.BUILDS)
def test_host_form_equals_the_model_bit_for_bit(tmp_path, build):
    exe = HF.build(tmp_path, "pnp_solver_mirror", build)
    (tmp_path / "problem.bin").write_bytes(_problem())
    HF.run(exe, str(tmp_path / "problem.bin"), str(tmp_path / "out.bin"))
    r = _Reader((tmp_path / "out.bin").read_bytes())
    for name in SCENES:
        s, m = S.scene(name), S.model(name)
        cap, mi, words = s["capacity"], s["max_its"], (s["capacity"] + 31) // 32
        head = tuple(int(v) for v in r.take(np.int32, 5))
        assert head == (m["status"], m["n_corr"], m["n_its"], m["n_events"], m["exhausted"]), name
        assert np.array_equal(r.take(np.int32, cap + 1), s["its_for_n"]), name
        assert np.array_equal(r.take(np.int32, 2 * cap).reshape(cap, 2), m["corr"]), name
        assert np.array_equal(r.take(np.int32, 4 * mi).reshape(mi, 4), m["sets"]), name
        assert np.array_equal(r.take(np.int32, mi), m["events"]), name
        hyp = r.take(M.HYP_DTYPE, mi)
        assert np.array_equal(hyp["n_inliers"], m["hyp"]["n_inliers"]), (name, hyp["n_inliers"][:12], m["hyp"]["n_inliers"][:12])
        _same_records(hyp, m["hyp"], name, "hypotheses")
        assert np.array_equal(r.take(np.uint32, mi * words).reshape(mi, words), m["bits"]), name
        _same_records(r.take(M.REFINED_DTYPE, mi), m["refined"], name, "refinements")
        assert np.array_equal(r.take(np.uint32, mi * words).reshape(mi, words), m["refined_bits"]), name
        n_its, N = m["n_its"], m["n_corr"]
        min_c, its = M.min_inliers_for(N, s["min_inliers"], s["epsilon"]), int(s["its_for_n"][N])
        for step in (1, 5, 300):
            want = literal_walk(N, m["hyp"]["n_inliers"][:n_its], m["refined"]["ok"][:n_its], m["refined"]["n_inliers"][:n_its], min_c, its, step)
            got = _replay_log(r)
            assert [(a, bool(b), c, e, f) for a, b, c, _, e, f in got] == want, (name, step, got, want)
            assert all(d == c for _, _, c, d, _, _ in got), (name, step)       # one keypoint per inlier correspondence
        before, after = r.take(np.int32, 2)
        assert (before, after) == (0, 0) if n_its == 0 else before < after <= max(before, its) + 15, (name, before, after)   # three more iterate(5), beyond the rows
    for N, its, mn, step, counts, ok in REPLAYS:
        got = _replay_log(r)
        assert [(a, bool(b), c, e, f) for a, b, c, _, e, f in got] == literal_walk(N, counts, ok, counts, mn, its, step), (N, its, mn, step, counts, got)
    assert r.at == len(r.d)
