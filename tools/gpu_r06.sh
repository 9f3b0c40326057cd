# Round-6 GPU session (run via gpurun from the repo root):
#   bash tools/gpu_r06.sh "<test files or ->" [bench|full|smoke] ...
set -o pipefail
cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-bench_out}; mkdir -p "$OUT"     # OUT: the folder the logs and JSON lines go to
FIRST=$1; shift
if [ "$FIRST" != "-" ]; then
  timeout -k 10 600 python -u -m pytest $FIRST -m gpu -x -v --timeout 200 --timeout-method thread > $OUT/pytest_first.log 2>&1 || { echo PYTEST_FIRST_FAIL; tail -40 $OUT/pytest_first.log; exit 1; }
  tail -1 $OUT/pytest_first.log
fi
for p in "$@"; do
  case $p in
    full) timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > $OUT/pytest_gpu.log 2>&1 || { echo PYTEST_FAIL; tail -40 $OUT/pytest_gpu.log; exit 1; }
          tail -1 $OUT/pytest_gpu.log ;;
    smoke) timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 || { echo SMOKE_FAIL; tail -20 $OUT/smoke.log; exit 1; }; tail -1 $OUT/smoke.log ;;
    bench) timeout -k 10 600 python3 -u bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/bench.json 2> $OUT/bench.err || { echo BENCH_FAIL; tail -30 $OUT/bench.err; exit 1; }
           wc -c $OUT/bench.json; cat $OUT/bench.json ;;
    bench:*) timeout -k 10 600 python3 -u bench.py ${p#bench:} > $OUT/bench_x.json 2> $OUT/bench_x.err || { echo BENCHX_FAIL; tail -30 $OUT/bench_x.err; exit 1; }
           cat $OUT/bench_x.json ;;
    py:*) timeout -k 10 600 python3 -u ${p#py:} > $OUT/py.log 2>&1 || { echo PY_FAIL; tail -30 $OUT/py.log; exit 1; }; tail -30 $OUT/py.log ;;
  esac
done
