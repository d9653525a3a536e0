#!/bin/bash
out=${BENCH_OUT:-bench_out}  # where the runs' lines and logs go
mkdir -p $out/r04
s=$(date +%s.%N)
python3 bench.py --full --steps 20 --warmup 5 > $out/r04/bench_timed.json 2> $out/r04/bench_timed.err; echo "rc=$?"
e=$(date +%s.%N)
echo "wall $(echo "$e - $s" | bc) s"
python3 -c "
import json; d=json.loads(open('$out/r04/bench_timed.json').read().strip().splitlines()[-1]); print(d['value'], d['config']['host_fed']['overlapped'], d['config']['pipelined']['value'], d['config']['secondary'].get('error'))"
