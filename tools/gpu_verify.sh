# Re-entry verification: GPU parity tests, smoke, the full bench line, kernel-trace stats of the
# NS step and the full-graph leg. Logs and traces under $REGNN_OUT (default bench_out/).
cd "$(dirname "$0")/.." && export TMPDIR=/tmp && OUT=${REGNN_OUT:-bench_out} && mkdir -p $OUT &&
tools/gpu_step.sh 900 $OUT/pytest_gpu.log python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread -p no:cacheprovider &&
tail -3 $OUT/pytest_gpu.log &&
tools/gpu_step.sh 300 $OUT/smoke.log python -c "import __graft_entry__ as g; g.smoke()" &&
tail -2 $OUT/smoke.log &&
tools/gpu_step.sh 900 $OUT/bench.log python bench.py --full &&
tail -1 $OUT/bench.log &&
tools/gpu_step.sh 900 $OUT/prof_mag.log rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_mag -o run -- python bench.py --full --steps 10 --warmup 2 --no-cpu-baseline
