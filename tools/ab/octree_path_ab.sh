#!/bin/bash
# usage: tools/ab/octree_path_ab.sh build                               (where hipcc is: no GPU needed)
#        tools/ab/octree_path_ab.sh run [step] [full] [trace] [timeline]   (on the GPU box, from the repository root; no phase named: all four)
# The quadtree's short passes off the workgroup barriers (tools/experiments/README.md "Quadtree: short passes without block barriers"):
#   parent.so       the parent commit's liborbfe.so      cuts_parent.so  its `make cuts` build (tools/ab/cuts.so of that checkout)
#   product.so      this tree's library                  cuts.so         this tree's `make cuts` build
# (build the parent from a checkout of that commit and copy the two files here under those names)
# `run` alternates the builds in ONE job on one GPU; a failing or timed-out step ends the job (nothing else is started on the GPU):
#   step      the --dump-outputs files of a plain run compared byte for byte with the parent's (sha256 of all of them recorded), then
#             `value` of the plain run (bench.py --gpus 1), parent and product alternating ROUNDS times; the verdict line says whether
#             every product run lies above the parent's best by more than 3x the spread (max - min) of the parent's own runs
#   full      one --full run per build (no CPU baseline, oracle check, host-fed or photograph part): config.single_frame, config.small_batch, config.pipelined
#   trace     rocprofv3 --kernel-trace --stats on the plain run, one run per build: median and mean of the octree3_kernel launches
#   timeline  tools/octree3_timeline.py on each cut-point build: the per-phase table of a workgroup
# Everything lands in $BENCH_OUT/octree_path (profiles/octree_path.json is made from it).  The product library is put back on exit.
set -o pipefail
cd "$(dirname "$0")/../.." || exit 1
ROUNDS=${ROUNDS:-4}
if [ "$1" = build ]; then
  make -j8 -C orbslam2_amd/csrc ARCH=gfx950 all cuts || exit 1
  cp orbslam2_amd/liborbfe.so tools/ab/product.so
  for f in parent cuts_parent; do [ -f tools/ab/$f.so ] || echo "tools/ab/$f.so is missing: build the parent commit and copy its library there"; done
  sha256sum tools/ab/parent.so tools/ab/product.so tools/ab/cuts_parent.so tools/ab/cuts.so
  exit 0
fi
[ "$1" = run ] || { echo "usage: $0 build | run [step] [full] [trace] [timeline]"; exit 1; }
shift
phases=${*:-step full trace timeline}
export TMPDIR=/tmp
out=${BENCH_OUT:-bench_out}/octree_path; mkdir -p $out
keep=$(mktemp); cp orbslam2_amd/liborbfe.so $keep
trap 'cp $keep orbslam2_amd/liborbfe.so; rm -f $keep' EXIT
use() { cp tools/ab/$1.so orbslam2_amd/liborbfe.so; }
fail() { echo "FAILED: $*"; exit 1; }
value() { # file tag log
  python3 -c "
import json; d = json.loads(open('$1').read().strip().splitlines()[-1]); print('$2', round(d['value'], 1), round(d['ms_per_step'], 5))" | tee -a $out/$3.txt
}
timeout -k 10 60 python3 -c "import torch; print(torch.cuda.get_device_name(0))" > $out/gpu.txt 2>/dev/null || fail no GPU
sha256sum tools/ab/parent.so tools/ab/product.so > $out/builds.txt
for ph in $phases; do case $ph in
step)
  for v in parent product; do
    use $v
    timeout -k 10 200 python3 bench.py --gpus 1 --dump-outputs $out/dump_$v > $out/dump_$v.json 2> $out/dump_$v.err || fail dump $v
    (cd $out/dump_$v && sha256sum *) > $out/outputs_sha256_$v.txt
    rm -rf $out/dump_$v
  done
  n=$(wc -l < $out/outputs_sha256_parent.txt)
  if cmp -s $out/outputs_sha256_parent.txt $out/outputs_sha256_product.txt; then same=1; else same=0; fi
  echo "OUTPUTS files=$n identical=$same" | tee -a $out/outputs.txt
  [ $same -eq 1 ] || fail outputs differ
  for r in $(seq $ROUNDS); do for v in parent product; do
    use $v
    timeout -k 10 200 python3 bench.py --gpus 1 > $out/step_${v}_$r.json 2> $out/step.err || fail step $v
    value $out/step_${v}_$r.json "STEP $v $r" step
  done; done
  python3 -c "
import json
rd = lambda v: [json.loads(open('$out/step_%s_%d.json' % (v, r)).read().strip().splitlines()[-1])['value'] for r in range(1, $ROUNDS + 1)]
a, b = rd('parent'), rd('product')
spread = max(a) - min(a)
print('VERDICT parent %.1f..%.1f (spread %.1f, margin %.1f)  product %.1f..%.1f  mean gain %.2f %%  clears the margin in every alternation: %s'
      % (min(a), max(a), spread, 3 * spread, min(b), max(b), 100 * (sum(b) / sum(a) - 1), all(y > x + 3 * spread for x, y in zip(a, b))))" | tee -a $out/step.txt;;
full)
  for v in parent product; do
    use $v
    timeout -k 10 500 python3 bench.py --gpus 1 --full --cpu-pairs 0 --no-check --host-fed 0 --natural 0 > $out/full_$v.json 2> $out/full_$v.err || fail full $v
    python3 -c "
import json; c = json.loads(open('$out/full_$v.json').read().strip().splitlines()[-1])['config']
print('FULL $v', {k: c.get(k) for k in ('single_frame', 'small_batch', 'pipelined')})" | tee -a $out/full.txt
  done;;
trace)
  for v in parent product; do
    use $v; rm -rf $out/kt
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $out/kt -- python3 bench.py --gpus 1 > $out/kt.json 2> $out/kt.err || fail trace $v
    python3 -c "
import csv, sys
d = sorted((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in csv.DictReader(open(sys.argv[1])) if 'octree3_kernel' in r['Kernel_Name'])
print('TRACE $v octree3_kernel launches %d  median %.1f us  mean %.1f us  min %.1f us' % (len(d), d[len(d) // 2], sum(d) / len(d), d[0]))" "$(find $out/kt -name '*kernel_trace.csv' | head -1)" | tee -a $out/trace.txt || fail trace table $v
    cp "$(find $out/kt -name '*kernel_stats.csv' | head -1)" $out/kernel_stats_$v.csv
    rm -rf $out/kt
  done;;
timeline)
  for v in cuts_parent cuts; do
    use $v
    timeout -k 10 300 python3 tools/octree3_timeline.py > $out/timeline_$v.txt 2> $out/timeline.err || fail timeline $v
    grep -E "launch span|level [0-7] phases" $out/timeline_$v.txt | sed "s/^/TIMELINE $v /"
  done;;
*) fail "unknown phase $ph";;
esac; done
date -u +%Y-%m-%d > $out/date.txt
echo DONE
