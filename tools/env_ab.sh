# bench.py --workload $W under each environment setting of $CFGS (space-
# separated; "base" = none), alternating twice on one box; the runs' files go
# to $OUT (default bench_out)
set -e
W=${W:-flybase}
CFGS=${CFGS:-base}
OUT=${OUT:-bench_out}
mkdir -p $OUT
for rep in $(seq 1 ${REPS:-2}); do
  for cfg in $CFGS; do
    tag=$(echo "$cfg" | tr '=,' '__')
    if [ "$cfg" = "base" ]; then envs=""; else envs=$(echo "$cfg" | tr ',' ' '); fi
    o=$OUT/env_${W}_${tag}_$rep
    env $envs timeout -k 10 300 python bench.py --full --workload $W --steps 20 --warmup 5 --no-cpu-baseline --no-materialise --detail $o.json > $o.out 2> $o.err
    echo "$W $cfg rep $rep: $(tail -1 $o.out | python -c "import json,sys; d=json.loads(sys.stdin.read()); print(d['ms_per_step'], 'matched', d.get('step_ms_matched'), 'q2', (d.get('and_join_q2') or {}).get('us'), 'cart', (d.get('roofline') or {}).get('avg_launch_us'))")"
  done
done
