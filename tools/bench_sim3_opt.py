"""Latency of one orbfe_enqueue_optimize_sim3 call plus the stream synchronise, at 60 and at 300 correspondences between keyframes of
1500 and 1400 keypoint slots (the scenes corr60 / corr300 of tests/sim3_opt_scenes.py: a tenth gross outliers, so both optimize() calls
and both classifications run).  A host clock around enqueue + synchronise; every shape is warmed up first; the two shapes alternate over
several rounds so that a drift of the machine shows as a spread between rounds, not as a difference between the shapes.  Prints one JSON
line.  Needs a GPU: there is no CPU path.

    python tools/bench_sim3_opt.py [--reps 400] [--rounds 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import torch
    from orbslam2_amd import api
    from tests import sim3_opt_scenes as S
    from tests.device_arrays import context
    from tests.test_sim3_opt_device import _Call
    ctx = context(api)
    st = torch.cuda.Stream()
    out = {}
    calls = {name: _Call(api, S.scene(name)) for name in ("corr60", "corr300")}
    # d_match12 is in/out: a call on its own output finds the outliers already cleared.  Restore it (on the stream, outside the
    # timed window) so that every timed call does the first call's work.
    fresh = {name: torch.from_numpy(S.scene(name)["match12"].copy()).to("cuda:0") for name in calls}

    def once(name, timed=True):
        c = calls[name]
        with torch.cuda.stream(st):
            c.match.view.copy_(fresh[name])
        st.synchronize()
        t0 = time.perf_counter()
        c.enqueue(ctx, st)
        st.synchronize()
        return (time.perf_counter() - t0) * 1e6

    for name in calls:
        for _ in range(20):
            once(name)
        ref = S.model(name)
        got = calls[name].fetch()
        assert got["n_inliers"] == ref["n_inliers"] and got["status"] == 0, (name, got["n_inliers"], ref["n_inliers"])
    per_round = {name: [] for name in calls}
    for _ in range(a.rounds):
        for name in calls:
            per_round[name].append([once(name) for _ in range(a.reps)])
    for name, rounds in per_round.items():
        allt = [t for r in rounds for t in r]
        out[name] = dict(n_corr=int(S.model(name)["n_corr"]), n_inliers=int(S.model(name)["n_inliers"]), median_us=round(statistics.median(allt), 1),
                         mean_us=round(statistics.fmean(allt), 1), min_us=round(min(allt), 1), p95_us=round(sorted(allt)[int(0.95 * len(allt))], 1),
                         round_medians_us=[round(statistics.median(r), 1) for r in rounds], calls=len(allt))
    ctx.close()
    print(json.dumps(dict(bench="optimize_sim3_latency", what="enqueue + stream synchronise, host clock", **out)))


if __name__ == "__main__":
    main()
