#!/bin/bash
# usage: tools/ab/stereo_compact_ab.sh   (expects tools/ab/parent.so = the parent commit's liborbfe.so and tools/ab/new.so = the one under test)
# On one GPU, in one job, alternating: the --dump-outputs files of both builds compared byte for byte, stereo_match_kernel's average under
# a kernel trace (three alternations), the step with --repeat 8 (three), the other configurations of --full (two), and the SQ counters
# of the build under test in a run of their own.  Everything lands in $BENCH_OUT/stereo_compact (profiles/stereo_compact.json is made
# from it).  The product library is put back on exit.
set -o pipefail
export TMPDIR=/tmp
out=${BENCH_OUT:-bench_out}/stereo_compact; rm -rf $out; mkdir -p $out
keep=$(mktemp); cp orbslam2_amd/liborbfe.so $keep
trap 'cp $keep orbslam2_amd/liborbfe.so; rm -f $keep' EXIT
use() { cp tools/ab/$1.so orbslam2_amd/liborbfe.so; }
fail() { echo "FAILED: $*"; exit 1; }
timeout -k 10 60 python3 -c "import torch; print(torch.cuda.get_device_name(0))" > $out/gpu.txt 2>/dev/null
timeout -k 10 200 python3 -m pytest -x -q tests/test_gpu_stereo_compact.py tests/test_gpu_stereo_tail.py > $out/pytest_stereo.txt 2>&1 || fail stereo tests on the product library
tail -1 $out/pytest_stereo.txt
for v in parent new; do
  use $v
  python3 -c "import ctypes; l = ctypes.CDLL('orbslam2_amd/liborbfe.so'); l.orbfe_build_id.restype = ctypes.c_char_p; print('$v', l.orbfe_build_id().decode())" >> $out/build_ids.txt
  timeout -k 10 200 python3 bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs $out/dump_$v > $out/dump_$v.json 2> $out/dump_$v.err || fail dump $v
done
n=0; same=1
for f in $out/dump_parent/*.npy; do n=$((n+1)); cmp -s $f $out/dump_new/$(basename $f) || { same=0; echo "DIFFERS $(basename $f)"; }; done
[ $(ls $out/dump_new/*.npy | wc -l) -eq $n ] || same=0
echo "OUTPUTS files=$n identical=$same" | tee $out/outputs.txt
(cd $out/dump_new && sha256sum *.npy) > $out/outputs_sha256.txt
rm -rf $out/dump_parent $out/dump_new
[ $same -eq 1 ] || fail outputs differ
for r in 1 2 3; do for v in parent new; do
  use $v; rm -rf $out/kt
  timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $out/kt -- python3 bench.py --gpus 1 --steps 20 --warmup 5 > $out/kt.json 2> $out/kt.err || fail ktime $v
  f=$(find $out/kt -name "*kernel_stats.csv" | head -1)
  python3 -c "
import csv
for r in csv.DictReader(open('$f')):
    if 'stereo_match' in r['Name']: print('KTIME $v $r', r['Calls'], round(float(r['AverageNs'])/1000,3))" | tee -a $out/ktime.txt
  [ $r -eq 3 ] && cp $f $out/kernel_stats_$v.csv
  rm -rf $out/kt
done; done
for r in 1 2 3; do for v in parent new; do
  use $v
  timeout -k 10 300 python3 bench.py --gpus 1 --steps 20 --warmup 5 --repeat 8 > $out/step_${v}_$r.json 2> $out/step.err || fail step $v
  python3 -c "
import json; d = json.loads(open('$out/step_${v}_$r.json').read().strip().splitlines()[-1]); print('STEP $v $r', round(d['value'], 1), round(d['ms_per_step'], 5), d.get('config', {}).get('repeat'))" | tee -a $out/step.txt
done; done
for r in 1 2; do for v in parent new; do
  use $v
  timeout -k 10 500 python3 bench.py --gpus 1 --steps 20 --warmup 5 --full --cpu-pairs 0 --host-fed 0 --secondary 0 --no-check > $out/full_${v}_$r.json 2> $out/full.err || fail full $v
  python3 -c "
import json; d = json.loads(open('$out/full_${v}_$r.json').read().strip().splitlines()[-1]); c = d['config']
print('FULL $v $r value', round(d['value'], 1), 'natural', round(c['natural_image']['value'], 1), 'pipelined', round(c['pipelined']['value'], 1), 'small_batch', round(c['small_batch']['value'], 1))" | tee -a $out/full.txt
done; done
use new
timeout -k 10 300 rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVES SQ_WAVE_CYCLES SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAIT_INST_ANY SQ_ACTIVE_INST_VALU SQ_BUSY_CYCLES --output-format csv -d $out/pmc -- python3 bench.py --gpus 1 --steps 4 --warmup 2 > /dev/null 2> $out/pmc.err || fail pmc
f=$(find $out/pmc -name "*counter_collection.csv" | head -1)
python3 - "$f" <<'PY' | tee $out/pmc_new.txt
import csv, sys, collections
acc = collections.defaultdict(float); disp = set()
for r in csv.DictReader(open(sys.argv[1])):
    if "stereo_match" not in r["Kernel_Name"]: continue
    acc[r["Counter_Name"]] += float(r["Counter_Value"]); disp.add(r["Dispatch_Id"])
print("PMC new stereo_match_kernel n=%d" % len(disp), {a: round(b / len(disp), 1) for a, b in sorted(acc.items())})
PY
rm -rf $out/pmc
date -u +%Y-%m-%d > $out/date.txt
echo DONE
