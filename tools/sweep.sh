#!/bin/bash
# solve-kernel trace + points sweep (linearize roofline regime).  usage: tools/sweep.sh TAG   (outputs under $OUT_ROOT/TAG/)
TAG=${1:-sweep}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT_ROOT:-$ROOT/out}/$TAG
cd $ROOT && mkdir -p $OUT
HS_KTRACE=1 timeout -k 10 200 python bench.py --full --steps 5 --warmup 2 --no-cpu > $OUT/tr.json 2> $OUT/trace.txt || exit 1
grep "hs trace" $OUT/trace.txt | tail -24
for P in 2000 20000 200000; do
  timeout -k 10 200 python bench.py --full --steps 30 --warmup 3 --no-cpu --points $P > $OUT/p$P.json 2> $OUT/p$P.err || exit 1
  python3 -c "import json;d=json.load(open('$OUT/p$P.json'));print($P, d['config']['point_residuals'], round(d['value']/1e6,1), 'Mpres/s', round(d['ms_per_step'],4), 'ms/step lin', round(d['roofline']['avg_launch_ms'],4), 'ms', round(d['roofline']['achieved'],1), 'GB/s')"
done
