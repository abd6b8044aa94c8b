#!/bin/bash
# Full GPU pass: whole -m gpu suite (per-test timeout sized for the 2^24 cases), then the bench with --full
# (headline + roofline, secondaries, CPU baselines).  Logs go to $GM_OUT_DIR (default bench_out/).
#   bash tools/gpu_full.sh TAG
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${GM_OUT_DIR:-bench_out}
mkdir -p "$OUT"
export TMPDIR=/tmp
TAG=${1:-full}
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --durations=15 --timeout 400 --timeout-method thread > $OUT/${TAG}_tests.log 2>&1 || { tail -40 $OUT/${TAG}_tests.log; exit 1; }
tail -25 $OUT/${TAG}_tests.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" || exit 1
timeout -k 10 600 python -u bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err || { tail -30 $OUT/${TAG}_bench.err; exit 1; }
head -c 3000 $OUT/${TAG}_bench.json
