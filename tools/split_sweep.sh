#!/bin/bash
# accumulate split-size sweep: HS_ACC_SPLIT_POINTS in {64, 32, 16, 8}; trace + bench per setting (outputs under $OUT_ROOT/split/)
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT_ROOT:-$ROOT/out}/split
cd $ROOT && mkdir -p $OUT
for SP in 64 32 16 8; do
  HS_ACC_SPLIT_POINTS=$SP HS_KTRACE=1 timeout -k 10 120 python bench.py --full --steps 5 --warmup 2 --no-cpu > $OUT/tr$SP.json 2> $OUT/tr$SP.txt || exit 1
  HS_ACC_SPLIT_POINTS=$SP timeout -k 10 120 python bench.py --full --steps 200 --warmup 10 --no-cpu > $OUT/b$SP.json 2> $OUT/b$SP.err || exit 1
  echo "split $SP: $(python3 -c "import json;d=json.load(open('$OUT/b$SP.json'));print(round(d['ms_per_step']*1e3,2),'us/step')") $(grep -E 'accumulate   blocks|stitch       blocks' $OUT/tr$SP.txt | tr '\n' ' ')"
done
