#!/bin/bash
# the fresh-batch loop's region time against the number of steps (start-up and drain of the four-deep pipeline against its steady state)
# Usage: bash scripts/experiments/steps_sweep.sh <outdir>
OUT=${1:?usage: steps_sweep.sh <outdir>}; mkdir -p $OUT
for k in 20 40 80 160 320; do RAWDTW_BENCH_DUMP=1 timeout -k 10 300 python bench.py --full --no-cpu-baseline --modes-reads 0 --rounds 0 --steps $k > $OUT/st$k.json 2> $OUT/st$k.err; python3 -c "
import json; d=json.loads(open('$OUT/st$k.json').read().strip().splitlines()[-1]); print('steps $k', round(d['value_resident'],1), round(d['ms_per_step_resident'],4), d['repeats'], d['region_ms'], 'pcie', round(d['value_pcie'],1))"; done
