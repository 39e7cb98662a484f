#!/bin/bash
# GPU-box: default bench line, then the same command under rocprofv3 kernel trace.
set -o pipefail
BENCH_ARGS="--full ${BENCH_ARGS:-}"  # every leg of the line, not the headline run alone
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
mkdir -p gpurun_out
timeout -k 10 600 python bench.py ${BENCH_ARGS:-} > gpurun_out/bench.json 2> gpurun_out/bench.err || { tail -30 gpurun_out/bench.err; exit 1; }
cat gpurun_out/bench.json
if [ -n "${PROFILE:-}" ]; then
  export TMPDIR=/tmp
  timeout -k 10 600 rocprofv3 --kernel-trace --stats -d gpurun_out/prof -o run --output-format csv -- python3 bench.py --no-cpu-baseline ${BENCH_ARGS:-} > gpurun_out/prof_bench.json 2> gpurun_out/prof.err || { tail -20 gpurun_out/prof.err; exit 1; }
  find gpurun_out/prof -name "*stats*" | head
fi
