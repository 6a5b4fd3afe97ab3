# bench at several sizes (occupancy sweep): bash tools/sizes.sh "28 29 30" [extra bench args]
set -o pipefail
cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}  # where the logs and result lines go
mkdir -p $OUT
for n in $1; do
  timeout -k 10 300 python bench.py --full --steps 30 --warmup 10 --no-cpu-baseline --log2n $n ${@:2} > $OUT/size_$n.log 2>&1
  rc=$?; [ $rc -eq 0 ] || { tail -3 $OUT/size_$n.log; exit $rc; }
  python3 -c "import json; d=json.loads(open('$OUT/size_$n.log').read().strip().splitlines()[-1]); print('log2n $n', 'value', d['value'], 'enc', d['encode_ms'], 'dec', d['decode_ms'])"
done
