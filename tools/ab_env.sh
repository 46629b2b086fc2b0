#!/bin/bash
# A/B of environment settings on the NS bench, interleaved, 300 timed steps each:
#   tools/ab_env.sh REPS "ENV1" "ENV2" ...   (each ENV a space-separated VAR=value list, "-" = none)
# logs under $REGNN_OUT (default bench_out/)
cd "$(dirname "$0")/.." && export TMPDIR=/tmp && OUT=${REGNN_OUT:-bench_out} && mkdir -p $OUT
reps=$1; shift 1
for r in $(seq $reps); do
  for e in "$@"; do
    envs=""; [ "$e" != "-" ] && envs="$e"
    env $envs timeout -k 10 200 python bench.py --full --workload ns --no-full-batch --no-cpu-baseline --steps 300 ${AB_ARGS} > $OUT/ab.log 2>&1 || { tail -5 $OUT/ab.log; exit 1; }
    echo "[$e] $(grep '^{' $OUT/ab.log | python -c 'import json,sys; d=json.loads(sys.stdin.read()); print(round(d["ms_per_step"]*1000,1), "us", round(d["value"]/1e6,1), "M", d["ns_kernels_ms"])')"
  done
done
