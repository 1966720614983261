# A/B of the XCD-aware linearize block order (HS_XCD=0/1) at 2k / 200k / 2M, plus a FETCH_SIZE pass at 200k
ROOT=$(cd "$(dirname "$0")/.." && pwd)
O=${OUT_ROOT:-$ROOT/out}/${1:-xcd}
cd $ROOT && mkdir -p $O
for P in 2000 200000 2000000; do
  for X in 0 1; do
    HS_XCD=$X timeout -k 10 200 python bench.py --full --points $P --steps 30 --warmup 3 --no-cpu --no-phase-split > $O/p${P}_x$X.json 2>$O/p${P}_x$X.err || { echo "bench $P $X failed"; tail -5 $O/p${P}_x$X.err; exit 1; }
    python3 -c "import json;d=json.load(open('$O/p${P}_x$X.json'));r=d['roofline'];print('$P xcd=$X', round(d['ms_per_step']*1e3,2),'us/step', r['kernel'], round(r['avg_launch_ms']*1e3,2),'us frac', round(r['frac'],3))"
  done
done
cd /tmp && export TMPDIR=/tmp
for X in 0 1; do
  HS_XCD=$X timeout -s KILL 120 rocprofv3 --kernel-trace --stats --pmc FETCH_SIZE --output-format csv -d $O/pmc_x$X -o pmc -- python3 $ROOT/bench.py --full --points 200000 --steps 10 --warmup 2 --no-cpu --no-phase-split > $O/pmc_x$X.json 2> $O/pmc_x$X.err || { echo "pmc $X failed"; exit 1; }
done
echo done
