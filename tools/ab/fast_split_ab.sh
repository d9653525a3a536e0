#!/bin/bash
# usage: tools/ab/fast_split_ab.sh build                          (where hipcc is: no GPU needed)
#        tools/ab/fast_split_ab.sh run [step] [small] [full] [trace]   (on the GPU box, from the repository root; no phase named: all four)
# FAST's level 0 on the side stream beside the pyramid's launches (tools/experiments/README.md "FAST on level 0 beside the pyramid"):
#   parent.so   the parent commit's liborbfe.so (build it from a checkout of that commit and copy it to tools/ab/parent.so)
#   product.so  this tree's library; ORBFE_FAST_SPLIT=0 / 1 selects the single launch / the split at every batch size, unset = the planner's choice
# `run` alternates the builds in ONE job on one GPU; a failing or timed-out step ends the job (nothing else is started on the GPU):
#   step   the --dump-outputs files of a plain run compared byte for byte with the parent's, then `value` of the plain run
#          (bench.py --gpus 1) ROUNDS times each: parent, product with the split off, product as planned
#   small  plain runs of 8 pairs and of 1 pair with ORBFE_FAST_SPLIT=0 and =1, ROUNDS times each
#   full   one --full run per build (no CPU baseline, oracle check, host-fed or photograph part): config.pipelined, config.small_batch, config.single_frame
#   trace  rocprofv3 --kernel-trace --stats on the plain run, one run per build: per-kernel averages, and from the trace the wall interval
#          from the first resize launch of a step to the end of its last FAST launch against the sum of those kernels' own times
# Everything lands in $BENCH_OUT/fast_split (profiles/fast_split.json is made from it).  The product library is put back on exit.
set -o pipefail
cd "$(dirname "$0")/../.." || exit 1
ROUNDS=${ROUNDS:-3}
if [ "$1" = build ]; then
  make -j8 -C orbslam2_amd/csrc ARCH=gfx950 all || exit 1
  cp orbslam2_amd/liborbfe.so tools/ab/product.so
  [ -f tools/ab/parent.so ] || echo "tools/ab/parent.so is missing: build the parent commit and copy its liborbfe.so there"
  sha256sum tools/ab/*.so
  exit 0
fi
[ "$1" = run ] || { echo "usage: $0 build | run [step] [small] [full] [trace]"; exit 1; }
shift
phases=${*:-step small full trace}
export TMPDIR=/tmp
out=${BENCH_OUT:-bench_out}/fast_split; mkdir -p $out
keep=$(mktemp); cp orbslam2_amd/liborbfe.so $keep
trap 'cp $keep orbslam2_amd/liborbfe.so; rm -f $keep' EXIT
use() { cp tools/ab/$1.so orbslam2_amd/liborbfe.so; }
fail() { echo "FAILED: $*"; exit 1; }
# build name -> library and environment
lib_of() { case $1 in parent) echo parent;; *) echo product;; esac; }
env_of() { case $1 in off) echo ORBFE_FAST_SPLIT=0;; on) echo ORBFE_FAST_SPLIT=1;; *) echo ORBFE_AB_NONE=1;; esac; }
value() { # file tag
  python3 -c "
import json; d = json.loads(open('$1').read().strip().splitlines()[-1]); print('$2', round(d['value'], 1), round(d['ms_per_step'], 5))" | tee -a $out/$3.txt
}
timeout -k 10 60 python3 -c "import torch; print(torch.cuda.get_device_name(0))" > $out/gpu.txt 2>/dev/null || fail no GPU
for ph in $phases; do case $ph in
step)
  for v in parent off planned; do
    use $(lib_of $v)
    env $(env_of $v) timeout -k 10 200 python3 bench.py --gpus 1 --dump-outputs $out/dump_$v > $out/dump_$v.json 2> $out/dump_$v.err || fail dump $v
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
  for r in $(seq $ROUNDS); do for v in parent off planned; do
    use $(lib_of $v)
    env $(env_of $v) timeout -k 10 200 python3 bench.py --gpus 1 > $out/step_${v}_$r.json 2> $out/step.err || fail step $v
    value $out/step_${v}_$r.json "STEP $v $r" step
  done; done;;
small)
  use product
  for r in $(seq $ROUNDS); do for p in 8 1; do for v in off on; do
    env $(env_of $v) timeout -k 10 200 python3 bench.py --gpus 1 --pairs $p > $out/small_${p}_${v}_$r.json 2> $out/small.err || fail small $p $v
    value $out/small_${p}_${v}_$r.json "SMALL pairs=$p $v $r" small
  done; done; done;;
full)
  for v in parent planned; do
    use $(lib_of $v)
    env $(env_of $v) timeout -k 10 500 python3 bench.py --gpus 1 --full --cpu-pairs 0 --no-check --host-fed 0 --natural 0 > $out/full_$v.json 2> $out/full_$v.err || fail full $v
    python3 -c "
import json; c = json.loads(open('$out/full_$v.json').read().strip().splitlines()[-1])['config']
print('FULL $v', {k: c.get(k) for k in ('pipelined', 'small_batch', 'single_frame')})" | tee -a $out/full.txt
  done;;
trace)
  for v in parent planned; do
    use $(lib_of $v); rm -rf $out/kt
    env $(env_of $v) timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $out/kt -- python3 bench.py --gpus 1 > $out/kt.json 2> $out/kt.err || fail trace $v
    python3 tools/ab/fast_split_trace.py $v "$(find $out/kt -name '*kernel_trace.csv' | head -1)" | tee -a $out/trace.txt
    cp "$(find $out/kt -name '*kernel_stats.csv' | head -1)" $out/kernel_stats_$v.csv
    rm -rf $out/kt
  done;;
*) fail "unknown phase $ph";;
esac; done
date -u +%Y-%m-%d > $out/date.txt
echo DONE
