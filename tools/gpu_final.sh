# final measurement set: full bench lines (fp32 default with cpu_baseline, bf16), kernel
# stats and PMC HBM traffic of the mag-10x step. Bench logs under $REGNN_OUT (default bench_out/).
cd "$(dirname "$0")/.." && export TMPDIR=/tmp && OUT=${REGNN_OUT:-bench_out} && mkdir -p $OUT &&
tools/gpu_step.sh 900 $OUT/bench_full.log python bench.py --full &&
tools/gpu_step.sh 600 $OUT/bench_bf16.log python bench.py --full --dtype bf16 --no-cpu-baseline &&
tools/gpu_pmc2.sh
