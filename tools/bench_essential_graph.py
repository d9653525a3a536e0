"""Latency of one orbfe_enqueue_optimize_essential_graph call plus the stream synchronise on drifted rings with covisibility edges at 100,
500 and 2,000 keyframes (tests/essential_graph_scenes.py: closed by corrected Sim3s on the current keyframe and two neighbours, covisibles
k - 2 and k - 3, three points per keyframe).  A host clock around enqueue + synchronise; d_Tcw and d_pos are in/out, so they are restored
on the stream outside the timed window and every timed call does the first call's work; every shape is warmed up first; the shapes
alternate over several rounds so that a drift of the machine shows as a spread between rounds, not as a difference between the shapes.
The planner's host time is reported beside it (it runs once per loop closure, before the call).  Prints one JSON line.  Needs a GPU.

    python tools/bench_essential_graph.py [--reps 5] [--rounds 3] [--iterations 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"kfs_100": 100, "kfs_500": 500, "kfs_2000": 2000}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--free-scale", action="store_true", help="bFixScale = false (monocular)")
    a = ap.parse_args()
    import torch
    from orbslam2_amd import api
    from tests import essential_graph_scenes as SC
    from tests.device_arrays import context
    from tests.test_essential_graph_device import _Call
    ctx = context(api)
    st = torch.cuda.Stream()
    scenes = {name: dict(SC.closed_ring(n, covis=(2, 3)), iterations=a.iterations, fix_scale=not a.free_scale) for name, n in SHAPES.items()}
    plan_ms = {}
    for name, s in scenes.items():
        t0 = time.perf_counter()
        api.essential_graph_plan(len(s["Tcw"]), 0, s["edge_i"], s["edge_j"])
        plan_ms[name] = round((time.perf_counter() - t0) * 1e3, 3)
    calls = {name: _Call(api, s) for name, s in scenes.items()}
    fresh = {name: (torch.from_numpy(s["Tcw"].copy()).to("cuda:0"), torch.from_numpy(s["pos"].copy()).to("cuda:0")) for name, s in scenes.items()}
    torch.cuda.synchronize()

    def once(name):
        c = calls[name]
        with torch.cuda.stream(st):
            c.Tcw.view.copy_(fresh[name][0])
            c.pos.view.copy_(fresh[name][1])
        st.synchronize()
        t0 = time.perf_counter()
        c.enqueue(ctx, st)
        st.synchronize()
        return (time.perf_counter() - t0) * 1e3

    out, first = {}, {}
    for name in calls:
        for _ in range(a.warmup):
            once(name)
        got = calls[name].fetch()
        assert got["status"] == 0 and got["info"]["iterations"] > 0, (name, got["status"])
        first[name] = got
    per_round = {name: [] for name in calls}
    for _ in range(a.rounds):
        for name in calls:
            per_round[name].append([once(name) for _ in range(a.reps)])
    for name, rounds in per_round.items():
        got = calls[name].fetch()
        assert got["Tcw"].tobytes() == first[name]["Tcw"].tobytes() and got["pos"].tobytes() == first[name]["pos"].tobytes(), name   # the same work every time
        allt = [t for r in rounds for t in r]
        info = got["info"]
        out[name] = dict(keyframes=len(scenes[name]["Tcw"]), edges=int(info["n_active_edges"]), l_blocks=int(info["n_lblocks"]), in_lds=int(info["in_lds"]),
                         iterations=int(info["iterations"]), trials=int(info["trials"]), chi2_start=float(info["chi2_start"]), chi2_end=float(info["chi2_end"]),
                         plan_host_ms=plan_ms[name], median_ms=round(statistics.median(allt), 3), min_ms=round(min(allt), 3),
                         round_medians_ms=[round(statistics.median(r), 3) for r in rounds], calls=len(allt))
    ctx.close()
    print(json.dumps(dict(bench="optimize_essential_graph_latency", what="enqueue + stream synchronise, host clock", fix_scale=not a.free_scale, **out)))


if __name__ == "__main__":
    main()
