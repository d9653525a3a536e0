#!/bin/bash
# usage: tools/ab/describe_align_ab.sh build   (where hipcc is: no GPU needed)
#        tools/ab/describe_align_ab.sh run     (on the GPU box, from the repository root)
# describe_kernel's two measures (tools/experiments/README.md "describe: aligned raw loads, reversed image order"), each alone and both:
#   parent.so  the parent commit's liborbfe.so (build it from a checkout of that commit and copy it to tools/ab/parent.so)
#   a.so       ORBFE_DESC_ALIGN=1 ORBFE_DESC_REV=0      b.so   ORBFE_DESC_ALIGN=0 ORBFE_DESC_REV=1      ab.so  both
# `build` links the three (make describe-ab) from the product's objects with orbfe_describe.hip compiled under the switches.  `run`, on one GPU in one
# job, alternating the four: the --dump-outputs files compared byte for byte with the parent's, describe_kernel's average under
# a kernel trace and the step (`value`, --repeat 8) three times each, and the texture-addresser / L1 counters and FETCH_SIZE of
# describe_kernel in counter runs of their own.  Everything lands in $BENCH_OUT/describe_align (profiles/describe_align.json is made
# from it).  The product library is put back on exit.
set -o pipefail
cd "$(dirname "$0")/../.." || exit 1
VARIANTS="parent a b ab"
if [ "$1" = build ]; then
  make -j8 -C orbslam2_amd/csrc ARCH=gfx950 all describe-ab || exit 1
  [ -f tools/ab/parent.so ] || echo "tools/ab/parent.so is missing: build the parent commit and copy its liborbfe.so there"
  sha256sum tools/ab/*.so
  exit 0
fi
[ "$1" = run ] || { echo "usage: $0 build | run"; exit 1; }
export TMPDIR=/tmp
out=${BENCH_OUT:-bench_out}/describe_align; rm -rf $out; mkdir -p $out
keep=$(mktemp); cp orbslam2_amd/liborbfe.so $keep
trap 'cp $keep orbslam2_amd/liborbfe.so; rm -f $keep' EXIT
use() { cp tools/ab/$1.so orbslam2_amd/liborbfe.so; }
fail() { echo "FAILED: $*"; exit 1; }
timeout -k 10 60 python3 -c "import torch; print(torch.cuda.get_device_name(0))" > $out/gpu.txt 2>/dev/null || fail no GPU
timeout -k 10 300 python3 -m pytest -x -q tests/test_gpu_describe_align.py > $out/pytest_describe_align.txt 2>&1 || { tail -30 $out/pytest_describe_align.txt; fail describe tests on the product library; }
tail -1 $out/pytest_describe_align.txt
for v in $VARIANTS; do
  use $v
  echo "$v $(sha256sum tools/ab/$v.so | cut -c1-16) $(python3 -c "import ctypes; l = ctypes.CDLL('orbslam2_amd/liborbfe.so'); l.orbfe_build_id.restype = ctypes.c_char_p; print(l.orbfe_build_id().decode())")" >> $out/build_ids.txt
  timeout -k 10 200 python3 bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs $out/dump_$v > $out/dump_$v.json 2> $out/dump_$v.err || fail dump $v
  if [ $v != parent ]; then
    n=0; same=1
    for f in $out/dump_parent/*.npy; do n=$((n+1)); cmp -s $f $out/dump_$v/$(basename $f) || { same=0; echo "DIFFERS $v $(basename $f)"; }; done
    [ $(ls $out/dump_$v/*.npy | wc -l) -eq $n ] || same=0
    echo "OUTPUTS $v files=$n identical=$same" | tee -a $out/outputs.txt
    [ $same -eq 1 ] || fail outputs of $v differ
    rm -rf $out/dump_$v
  fi
done
(cd $out/dump_parent && sha256sum *.npy) > $out/outputs_sha256.txt
rm -rf $out/dump_parent
for r in 1 2 3; do for v in $VARIANTS; do
  use $v; rm -rf $out/kt
  timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $out/kt -- python3 bench.py --gpus 1 --steps 20 --warmup 5 > $out/kt.json 2> $out/kt.err || fail ktime $v
  f=$(find $out/kt -name "*kernel_stats.csv" | head -1)
  python3 -c "
import csv
for r in csv.DictReader(open('$f')):
    if any(k in r['Name'] for k in ('describe_kernel', 'stereo_match', 'fast_cell')): print('KTIME $v $r', r['Name'][:24], r['Calls'], round(float(r['AverageNs'])/1000,3))" | tee -a $out/ktime.txt
  [ $r -eq 3 ] && cp $f $out/kernel_stats_$v.csv
  rm -rf $out/kt
done; done
for r in 1 2 3; do for v in $VARIANTS; do
  use $v
  timeout -k 10 300 python3 bench.py --gpus 1 --steps 20 --warmup 5 --repeat 8 > $out/step_${v}_$r.json 2> $out/step.err || fail step $v
  python3 -c "
import json; d = json.loads(open('$out/step_${v}_$r.json').read().strip().splitlines()[-1]); print('STEP $v $r', round(d['value'], 1), round(d['ms_per_step'], 5), d.get('config', {}).get('repeat'))" | tee -a $out/step.txt
done; done
# counters, never beside a trace: the texture addresser and the L1 (profiles/r05_pmc_mem_ta.txt), then the L2's fetches
for set in "TA_BUSY_avr TA_TA_BUSY_sum TCP_TCC_READ_REQ_sum TCP_TOTAL_CACHE_ACCESSES_sum" "FETCH_SIZE"; do for v in $VARIANTS; do
  use $v; rm -rf $out/pmc
  timeout -k 10 300 rocprofv3 --pmc $set --output-format csv -d $out/pmc -- python3 bench.py --gpus 1 --steps 4 --warmup 2 > /dev/null 2> $out/pmc.err || fail pmc $v
  f=$(find $out/pmc -name "*counter_collection.csv" | head -1)
  python3 - "$f" $v <<'PY' | tee -a $out/pmc.txt
import csv, sys, collections
acc = collections.defaultdict(float); disp = set()
for r in csv.DictReader(open(sys.argv[1])):
    if "describe_kernel" not in r["Kernel_Name"]: continue
    acc[r["Counter_Name"]] += float(r["Counter_Value"]); disp.add(r["Dispatch_Id"])
print("PMC %s describe_kernel n=%d" % (sys.argv[2], len(disp)), {a: round(b / max(1, len(disp)), 1) for a, b in sorted(acc.items())})
PY
  rm -rf $out/pmc
done; done
date -u +%Y-%m-%d > $out/date.txt
echo DONE
