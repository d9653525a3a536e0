"""Scenes of the OptimizeEssentialGraph tests (tests/test_essential_graph_model.py, tests/test_essential_graph_device.py): keyframes on a
ring whose odometry drifts, closed by corrected Sim3s as LoopClosing::CorrectLoop forms them (src/LoopClosing.cc:436-467), with the edge
kinds of Optimizer::OptimizeEssentialGraph.  Keyframe 0 is the loop keyframe (fixed), keyframe n - 1 the current one.  Pure numpy."""
import numpy as np

from tests import sim3_opt_model as S3


def rot(axis, a):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def ring_truth(n, radius=2.0):
    """Tcw (float64 [n][4][4]) of n cameras on a circle, each turned along the tangent, with a little height and tilt."""
    out = []
    for k in range(n):
        a = 2 * np.pi * k / n
        Rwc = rot([0, 0, 1], a) @ rot([1, 0, 0], 0.1 * np.sin(3 * a))
        twc = np.array([radius * np.cos(a), radius * np.sin(a), 0.2 * np.sin(2 * a)])
        T = np.eye(4)
        T[:3, :3] = Rwc.T
        T[:3, 3] = -Rwc.T @ twc
        out.append(T)
    return np.array(out)


def drifted(truth, scale_step=0.985, yaw_step=0.012):
    """The odometry's poses: every relative motion of `truth` with its translation shrunk and a yaw error, chained from keyframe 0."""
    out = [truth[0].copy()]
    for k in range(1, len(truth)):
        rel = truth[k] @ np.linalg.inv(truth[k - 1])   # T_k,k-1
        rel[:3, :3] = rot([0, 0, 1], yaw_step) @ rel[:3, :3]
        rel[:3, 3] *= scale_step
        out.append(rel @ out[-1])
    return np.array(out)


def as_rows(T):
    return np.asarray(T, np.float64).reshape(-1, 16).astype(np.float32)


def sim3_of(T, s=1.0):
    return S3.sim3(T[:3, :3], T[:3, 3], s)


def ring_edges(n, covis=(2,), loop_pairs=((-1, 0),)):
    """(edge_i, edge_j, edge_kind): the loop connections first (kind 0), then per keyframe its parent k - 1 and its covisibles k - c."""
    ei, ej, ek = [], [], []
    for i, j in loop_pairs:
        ei.append(i % n); ej.append(j % n); ek.append(0)
    for k in range(n):
        if k >= 1:
            ei.append(k); ej.append(k - 1); ek.append(1)
        for c in covis:
            if k >= c:
                ei.append(k); ej.append(k - c); ek.append(1)
    return np.array(ei, np.int32), np.array(ej, np.int32), np.array(ek, np.uint8)


def closed_ring(n, scale=1.1, n_corrected=3, covis=(2,), seed=0):
    """A drifted ring of n keyframes closed at the current keyframe n - 1: the corrected Sim3 of the current keyframe is the truth with
    `scale`, its n_corrected - 1 predecessors are carried along (Sic * g2oScw), NonCorrectedSim3 holds their odometry poses.  Returns the
    keyword arguments of essential_graph_model.run / Context.optimize_essential_graph, with a few points per keyframe."""
    truth = ring_truth(n)
    odo = drifted(truth)
    Tcw = as_rows(odo)
    cur = n - 1
    g2oScw = sim3_of(truth[cur], scale)
    corrected, has_c = np.zeros((n, 8)), np.zeros(n, np.uint8)
    noncorrected, has_n = np.zeros((n, 8)), np.zeros(n, np.uint8)
    odo32 = Tcw.astype(np.float64).reshape(-1, 4, 4)
    for k in range(max(cur - n_corrected + 1, 1), n):
        Siw = sim3_of(odo32[k])
        Sic = S3.sim3_mul(Siw, S3.sim3_inverse(sim3_of(odo32[cur])))
        corrected[k] = S3.pack(S3.sim3_mul(Sic, g2oScw)); has_c[k] = 1
        noncorrected[k] = S3.pack(Siw); has_n[k] = 1
    loop_pairs = [(cur, 0)] + ([(cur - 1, 0)] if n_corrected > 1 and n > 3 else [])
    ei, ej, ek = ring_edges(n, covis, loop_pairs)
    rng = np.random.default_rng(seed)
    n_pts = 3 * n + 1
    pos = rng.uniform(-3, 3, (n_pts, 3)).astype(np.float32)
    pt_ref = (np.arange(n_pts) % n).astype(np.int32)
    pt_valid = (np.arange(n_pts) % 5 != 3).astype(np.uint8)
    return dict(Tcw=Tcw, fixed_kf=0, edge_i=ei, edge_j=ej, edge_kind=ek, corrected=corrected, has_corrected=has_c, noncorrected=noncorrected,
                has_noncorrected=has_n, pos=pos, pt_ref=pt_ref, pt_valid=pt_valid)


def noiseless_ring(n, seed=1):
    """NonCorrectedSim3 = the truth for every keyframe and only kind-1 edges: the measurements are consistent, the initial poses are
    the truth perturbed, and the optimum has zero error."""
    truth = ring_truth(n)
    rng = np.random.default_rng(seed)
    pert = []
    for k in range(n):
        T = truth[k].copy()
        if k:
            T[:3, :3] = rot(rng.normal(size=3), 0.03) @ T[:3, :3]
            T[:3, 3] += rng.normal(scale=0.03, size=3)
        pert.append(T)
    ei, ej, ek = ring_edges(n, (2,), ())
    ei = np.append(ei, n - 1).astype(np.int32); ej = np.append(ej, 0).astype(np.int32); ek = np.append(ek, 1).astype(np.uint8)  # closes the ring
    non = np.array([S3.pack(sim3_of(T)) for T in truth])
    return dict(Tcw=as_rows(pert), fixed_kf=0, edge_i=ei, edge_j=ej, edge_kind=ek, noncorrected=non, has_noncorrected=np.ones(n, np.uint8))


def _with_edges(sc, extra):
    """sc with (i, j, kind) triples appended."""
    ei, ej, ek = (list(sc[k]) for k in ("edge_i", "edge_j", "edge_kind"))
    for i, j, k in extra:
        ei.append(i); ej.append(j); ek.append(k)
    return dict(sc, edge_i=np.array(ei, np.int32), edge_j=np.array(ej, np.int32), edge_kind=np.array(ek, np.uint8))


def _pad_edges(sc, n_edges):
    """sc with duplicates of its own kind-1 edges, some of them reversed, up to n_edges edges."""
    base = [(int(i), int(j)) for i, j, k in zip(sc["edge_i"], sc["edge_j"], sc["edge_kind"]) if k == 1]
    extra = []
    for q in range(n_edges - len(sc["edge_i"])):
        i, j = base[(7 * q) % len(base)]
        extra.append((j, i, 1) if q % 3 == 0 else (i, j, 1))
    return _with_edges(sc, extra)


THREADS = 256   # EG_THREADS of orbfe_essential_blocks.hpp: the stride of every loop of the one workgroup

SCENES = {
    # name: (builder, iterations, fix_scale)
    "two": (lambda: dict(closed_ring(2, n_corrected=1, covis=()), **dict(zip(("edge_i", "edge_j", "edge_kind"), ring_edges(2, (), ())))), 1, False),
    "chain3": (lambda: dict(closed_ring(3, n_corrected=2, covis=()), **dict(zip(("edge_i", "edge_j", "edge_kind"), ring_edges(3, (), ())))), 1, False),
    "ring6": (lambda: closed_ring(6), 20, False),
    "ring6_fix_scale": (lambda: closed_ring(6), 20, True),
    "covis40": (lambda: closed_ring(40, covis=(2, 3)), 20, False),
    # three iterations: from the fourth on the chi2 gain is below 1e-12 of chi2 and the stop rules act on rounding
    "covis40_fix_scale": (lambda: closed_ring(40, covis=(2, 3)), 3, True),
    # one iteration: in this chain of 300 the numeric Jacobians' noise (7e-9 between two libms) moves the MODEL's own result by 4e-7
    # after one iteration, 1.5e-4 after two and 3.3e-4 after three: later iterations compare noise, not kernels
    "hbm300": (lambda: closed_ring(300), 1, True),
    "dup_rev": (lambda: _pad_edges(closed_ring(8), 40), 20, True),
    # the strides: keyframes (vertices, recovery), keyframes x 15 (perturbation tables), free keyframes x 7 (b, x), edges
    "kfs_255": (lambda: closed_ring(255, covis=()), 1, True), "kfs_256": (lambda: closed_ring(256, covis=()), 1, True),
    "kfs_257": (lambda: closed_ring(257, covis=()), 1, True),
    "kfs_17": (lambda: closed_ring(17), 2, True), "kfs_18": (lambda: closed_ring(18), 2, True),
    "kfs_37": (lambda: closed_ring(37), 2, True), "kfs_38": (lambda: closed_ring(38), 2, True),
    "edges_255": (lambda: _pad_edges(closed_ring(60), 255), 1, True), "edges_256": (lambda: _pad_edges(closed_ring(60), 256), 1, True),
    "edges_257": (lambda: _pad_edges(closed_ring(60), 257), 1, True),
    "no_points": (lambda: dict(closed_ring(6), pos=np.zeros((0, 3), np.float32), pt_ref=np.zeros(0, np.int32), pt_valid=np.zeros(0, np.uint8)), 2, True),
}


def faulty():
    """closed_ring(8) with three edges whose indices are faulty, a NaN in the corrected Sim3 of keyframe 6 and two points whose keyframe
    index lies outside the map."""
    sc = _with_edges(closed_ring(8), [(8, 1, 1), (2, -1, 0), (3, 3, 1)])
    sc["corrected"] = sc["corrected"].copy()
    sc["corrected"][6, 5] = np.nan
    sc["pt_ref"] = sc["pt_ref"].copy()
    sc["pt_ref"][0], sc["pt_ref"][1] = 8, -1   # both valid points
    return sc


SCENES["faulty"] = (faulty, 4, True)


def scene(name):
    build, iterations, fix_scale = SCENES[name]
    return dict(build(), iterations=iterations, fix_scale=fix_scale)
