#!/usr/bin/env python3
"""usage: fast_split_trace.py TAG kernel_trace.csv   (rocprofv3 --kernel-trace --output-format csv of a plain bench.py run)
Per step (the kernels up to and including a stereo_median_kernel): the wall interval from the start of the first pyramid launch to
the end of the last fast_cell_kernel, the sum of those kernels' own durations, and how long a fast_cell_kernel ran while a pyramid
launch was running.  Prints the medians over the last 20 steps, in microseconds."""
import csv
import statistics
import sys

tag, path = sys.argv[1], sys.argv[2]
rows = []
for r in csv.DictReader(open(path)):
    name = r.get("Kernel_Name") or r.get("Name")
    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name))
rows.sort()
steps, cur = [], []
for s, e, n in rows:
    cur.append((s, e, n))
    if "stereo_median_kernel" in n:
        steps.append(cur)
        cur = []
out = []
for st in steps[-20:]:
    pyr = [(s, e) for s, e, n in st if n.startswith(("pyr_", "void pyr_"))]
    fast = [(s, e) for s, e, n in st if "fast_cell_kernel" in n]
    if not pyr or not fast:
        continue
    wall = max(e for _, e in fast) - min(s for s, _ in pyr)
    own = sum(e - s for s, e in pyr + fast)
    both = sum(max(0, min(fe, pe) - max(fs, ps)) for fs, fe in fast for ps, pe in pyr)
    whole = st[-1][1] - min(s for s, _, _ in st)
    out.append((wall, own, both, len(pyr), len(fast), whole, [round((e - s) / 1e3, 1) for s, e in fast]))
if not out:
    sys.exit("no complete step in the trace")
med = lambda k: round(statistics.median(o[k] for o in out) / 1e3, 1)
print("TRACE %s steps=%d pyramid_launches=%d fast_launches=%d first_resize_to_last_fast_us=%s sum_of_kernel_times_us=%s fast_beside_pyramid_us=%s step_us=%s fast_us_last_step=%s"
      % (tag, len(out), out[-1][3], out[-1][4], med(0), med(1), med(2), med(5), out[-1][6]))
