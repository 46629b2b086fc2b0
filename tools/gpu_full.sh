# Full GPU verification: every -m gpu test, smoke() and the full bench line (NS step with its
# per-kernel figures + full-batch roofline leg + CPU baseline). Logs under $REGNN_OUT (default
# bench_out/).
cd "$(dirname "$0")/.." && export TMPDIR=/tmp && OUT=${REGNN_OUT:-bench_out} && mkdir -p $OUT &&
tools/gpu_step.sh 900 $OUT/pytest_gpu.log python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread -p no:cacheprovider &&
tail -3 $OUT/pytest_gpu.log && grep -q " passed" $OUT/pytest_gpu.log && ! grep -q " failed" $OUT/pytest_gpu.log &&
tools/gpu_step.sh 300 $OUT/smoke.log python -c "import __graft_entry__ as g; g.smoke()" &&
tail -2 $OUT/smoke.log &&
tools/gpu_step.sh 900 $OUT/bench.log python bench.py --full &&
tail -1 $OUT/bench.log
