#!/bin/bash
# BA parity tests + per-phase kernel trace + short bench.  usage: tools/ba_check.sh TAG   (outputs under $OUT_ROOT/TAG/)
TAG=${1:-bac}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT_ROOT:-$ROOT/out}/$TAG
cd $ROOT && mkdir -p $OUT
timeout -k 10 300 python -u -m pytest tests/test_gpu_ba.py -m gpu -x -v --timeout 120 --timeout-method thread > $OUT/pytest.txt 2>&1
rc=$?; echo "pytest rc=$rc"; tail -15 $OUT/pytest.txt; [ $rc -ne 0 ] && exit $rc
HS_KTRACE=1 timeout -k 10 200 python bench.py --full --steps 5 --warmup 2 --no-cpu > $OUT/tr.json 2> $OUT/trace.txt || exit 1
grep "hs trace" $OUT/trace.txt | tail -24
timeout -k 10 200 python bench.py --full --steps 200 --warmup 10 --no-cpu > $OUT/b.json 2> $OUT/b.err || exit 1
python3 -c "import json;d=json.load(open('$OUT/b.json'));print(round(d['value']/1e6,2), 'Mpres/s', round(d['ms_per_step']*1e3,2), 'us/step; lin', round(d['roofline']['avg_launch_ms']*1e3,2), 'us')"
