out=${BENCH_OUT:-bench_out}  # where the runs' lines and logs go
mkdir -p $out
for d in 1 3 4 0; do
  ORBFE_FAST_DBG=$d timeout -k 10 120 python bench.py --full --cpu-pairs 0 --pipelined 0 --small-batch 0 --natural 0 --host-fed 0 --secondary 0 --no-check --steps 10 > $out/fd$d.json 2> $out/fd$d.err
  python -c "
import json;d=json.loads(open('$out/fd$d.json').read().strip().splitlines()[-1]);print($d, d['roofline']['stage_ms_per_step_summed_over_groups']['fast'])"
done
