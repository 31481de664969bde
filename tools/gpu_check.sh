#!/bin/bash
# On the GPU box: the -m gpu suite, a kernel-trace summary of the bench, and two bench lines.  Every GPU step under a time
# limit of its own; the first that fails ends the script.  usage: bash tools/gpu_check.sh <dir/tag> [kernel rows]
# (the suite's log, the trace and its log go to <dir/tag>_suite.log, <dir/tag>_stats/ and <dir/tag>_stats.log)
set -o pipefail
tag=${1:-chk}
export TMPDIR=/tmp
bench_line() {
  timeout -k 10 200 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline | python -c "
import json, sys; d=json.loads(sys.stdin.readline()); print(round(d['ms_per_step'],4), round(d['device_ms_per_step'],4), {k[3:]: round(v,4) for k,v in d['stage_ms'].items()})"
}
{ timeout -k 10 1100 python -m pytest tests -m gpu -x -q > ${tag}_suite.log 2>&1; rc=$?; echo "pytest rc=$rc"; tail -4 ${tag}_suite.log; [ $rc -eq 0 ]; } &&
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d ${tag}_stats -- python3 bench.py --steps 5 --warmup 2 --no-cpu-baseline > ${tag}_stats.log 2>&1 &&
python -c "
import sys; sys.path.insert(0, 'tools'); import ab
for name, calls, us in ab.kstats(sys.argv[1])[:int(sys.argv[2])]: print('%-100s %5d %9.1f us' % (name[:100], calls, us))" ${tag}_stats ${2:-14} &&
bench_line && bench_line
