export TMPDIR=/tmp
OUT=${1:?output directory}
mkdir -p $OUT
timeout -k 10 300 python bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --breakdown > $OUT/bench.json 2> $OUT/breakdown.txt || exit $?
for nb in 512 2048; do
  FVC_GDN_BLOCKS=$nb timeout -k 10 240 python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $OUT/gb_$nb.json 2>/dev/null || exit $?
  python -c "
import json; d=json.loads(open('$OUT/gb_$nb.json').read().strip().splitlines()[-1]); h=d['hbm_kernels']
print('blocks=$nb', d['value'], {k: (h[k]['gb_per_s'], h[k]['ms_per_pframe']) for k in ('gdn', 'gdn+tap')})"
done
