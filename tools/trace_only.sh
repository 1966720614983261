ROOT=$(cd "$(dirname "$0")/.." && pwd); OUT=${OUT_ROOT:-$ROOT/out}/tr
cd $ROOT && mkdir -p $OUT && HS_KTRACE=1 timeout -k 10 200 python bench.py --full --steps 5 --warmup 2 --no-cpu > $OUT/b.json 2> $OUT/trace.txt; grep "hs trace" $OUT/trace.txt | tail -30
