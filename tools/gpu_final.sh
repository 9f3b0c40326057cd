# Round-end check at HEAD (run via gpurun from the repo root): the whole -m gpu
# suite, smoke(), then the default bench -- the driver's own sequence.
set -o pipefail
cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-bench_out}; mkdir -p "$OUT"     # OUT: the folder the logs and JSON lines go to
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > $OUT/pytest.log 2>&1 || { echo PYTEST_FAIL; tail -40 $OUT/pytest.log; exit 1; }
tail -n 1 $OUT/pytest.log
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $OUT/smoke.log 2>&1 || { echo SMOKE_FAIL; tail -20 $OUT/smoke.log; exit 1; }
tail -n 1 $OUT/smoke.log
timeout -k 10 600 python -u bench.py --full > $OUT/bench.json 2> $OUT/bench.err || { echo BENCH_FAIL; tail -30 $OUT/bench.err; exit 1; }
python3 tools/bench_summary.py $OUT/bench.json || true
