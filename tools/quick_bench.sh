#!/bin/bash
# quick GPU timing: tests + bench with and without per-kernel HIP events + trace (outputs under $OUT_ROOT/qb/)
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT_ROOT:-$ROOT/out}/qb
cd $ROOT && mkdir -p $OUT
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > $OUT/pytest.txt 2>&1; echo "pytest rc=$?"; tail -3 $OUT/pytest.txt
timeout -k 10 200 python bench.py --full --steps 200 --warmup 10 --no-cpu > $OUT/ev.json 2>$OUT/ev.err || exit 1
HS_EVENT_TIMING=0 timeout -k 10 200 python bench.py --full --steps 200 --warmup 10 --no-cpu > $OUT/noev.json 2>$OUT/noev.err || exit 1
HS_KTRACE=1 timeout -k 10 200 python bench.py --full --steps 5 --warmup 2 --no-cpu > $OUT/tr.json 2> $OUT/trace.txt || exit 1
python3 -c "
import json
for f in ('ev','noev'):
    d=json.load(open('$OUT/%s.json'%f)); print(f, d['value'], d['ms_per_step'], d['phase_ms_per_step'])"
grep "hs trace" $OUT/trace.txt | tail -24
