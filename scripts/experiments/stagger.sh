# Usage: bash scripts/experiments/stagger.sh <outdir>
OUT=${1:?usage: stagger.sh <outdir>}; mkdir -p $OUT
for sg in 0 60 120 200; do RAWDTW_BENCH_DUMP=1 timeout -k 10 300 python bench.py --full --no-cpu-baseline --modes-reads 0 --rounds 0 --steps 80 --stagger-us $sg > $OUT/sg$sg.json 2> $OUT/sg$sg.err; echo "stagger $sg"; grep regions_ms $OUT/sg$sg.err | head -1 | cut -c1-260; done
