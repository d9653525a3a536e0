#!/usr/bin/env python3
"""Cycle breakdown of one orbfe_enqueue_local_bundle_adjustment call per shape of tools/bench_lba.py, on the instrumented build
(make -C orbslam2_amd/csrc lba-timing: -DORBFE_LBA_TIMING, clock64 of thread 0 around every phase; never shipped).  Prints one JSON line."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ["vertices, edges, sort", "error passes", "per-point linearisation", "Hpp walk", "Dinv and Hpl Dinv", "Schur rows", "LDLT",
         "landmark step, update, accept"]


def main():
    import torch
    from orbslam2_amd import api
    api.LIB_PATH = os.path.join(ROOT, "tools", "ab", "lba_timing.so")
    from tests import lba_scenes as S
    from tests.device_arrays import context
    from tests.test_lba_device import _Call
    from tools.bench_lba import SHAPES
    ctx = context(api)
    st = torch.cuda.Stream()
    out = {}
    cyc = (C.c_longlong * 8)()
    for name, spec in SHAPES.items():
        s = S.make(**spec)
        for k in range(2):              # the second call is the warm one
            c = _Call(api, s)
            assert ctx.L.orbfe_lba_debug_cycles(cyc, 1) == 0
            c.enqueue(ctx, st)
            st.synchronize()
            assert ctx.L.orbfe_lba_debug_cycles(cyc, 1) == 0
        total = float(sum(cyc))
        got = c.fetch()
        out[name] = dict(iterations=got["info"]["iterations"].tolist(), trials=got["info"]["trials"].tolist(), cycles=int(total),
                         share={n: round(cyc[i] / total, 4) for i, n in enumerate(NAMES)})
    ctx.close()
    print(json.dumps(dict(bench="local_bundle_adjustment_phases", **out)))


if __name__ == "__main__":
    main()
