"""Latency of one orbfe_enqueue_local_bundle_adjustment call plus the stream synchronise at two shapes: 10 local + 10 fixed keyframes
with 1000 points (small), and 30 + 30 with 5000 points and about 30 000 edges (large; the reduced system of 30 free keyframes lives in
HBM).  Scenes of tests/lba_scenes.py: a tenth gross outliers, so both optimize() calls and both classifications run.  A host clock
around enqueue + synchronise; d_Tcw and d_pos are in/out, so they are restored on the stream outside the timed window and every timed
call does the first call's work; every shape is warmed up first; the two shapes alternate over several rounds so that a drift of the
machine shows as a spread between rounds, not as a difference between the shapes.  Prints one JSON line.  Needs a GPU: there is no CPU
path.

    python tools/bench_lba.py [--reps 20] [--rounds 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {
    "small": dict(seed=41, roles=[1] * 10 + [3] * 10, n_pts=1000, slots=600, views=6, spacing=0.15),
    "large": dict(seed=42, roles=[1] * 30 + [3] * 30, n_pts=5000, slots=1000, views=6, spacing=0.05),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    from orbslam2_amd import api
    from tests import lba_scenes as S
    from tests.device_arrays import context
    from tests.test_lba_device import _Call
    ctx = context(api)
    st = torch.cuda.Stream()
    scenes = {name: S.make(**spec) for name, spec in SHAPES.items()}
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
        assert got["status"] == 0 and got["info"]["iterations"][0] > 0, (name, got["status"])
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
        out[name] = dict(keyframes=len(scenes[name]["role"]), free=int(info["n_free"]), points=int(info["n_points"]),
                         edges=int(info["n_mono"]) + int(info["n_stereo"]), erased=got["n_erase"], iterations=info["iterations"].tolist(),
                         trials=info["trials"].tolist(), median_ms=round(statistics.median(allt), 3), min_ms=round(min(allt), 3),
                         p95_ms=round(sorted(allt)[int(0.95 * len(allt))], 3), round_medians_ms=[round(statistics.median(r), 3) for r in rounds],
                         calls=len(allt))
    ctx.close()
    print(json.dumps(dict(bench="local_bundle_adjustment_latency", what="enqueue + stream synchronise, host clock", **out)))


if __name__ == "__main__":
    main()
