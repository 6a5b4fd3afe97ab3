# C3 over chunk lengths (sweep 1024-16384): one bench line each.
set -o pipefail
cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}  # where the logs and result lines go
mkdir -p $OUT
: > $OUT/chunk_sweep.jsonl
for L in 1024 2048 4096 8192 16384; do
  timeout -k 10 200 python3 bench.py --full --chunk-len $L --steps 15 --warmup 8 --no-cpu-baseline --no-dense > $OUT/sweep_$L.log 2>&1 || { tail -3 $OUT/sweep_$L.log; exit 1; }
  grep '^{' $OUT/sweep_$L.log >> $OUT/chunk_sweep.jsonl
done
echo done
