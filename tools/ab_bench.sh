#!/bin/bash
# A/B of library builds on the headline IN THE BENCH CONTEXT (GPU box): alternating `bench.py --no-extras` processes,
# one pipelined stream object per process (several pipelined objects in one process share hardware queues and stop
# overlapping: profiles/r03_notes.md).   usage: tools/ab_bench.sh <rounds> <lib> [<lib> ...]   lib = "-" (the tree's
# build) or a variant name under yagi_amd/variants/.  The first lib runs once more after the last round (first and
# last).  Every bench process has its own time limit, and the first one that fails, faults or hangs ends the script:
# nothing more is started on that GPU.
set -o pipefail
rounds=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
one() {
  local lib=$1
  if [ "$lib" != "-" ]; then export YAGI_HIP_LIB=$root/yagi_amd/variants/libyagi_$lib.so; else unset YAGI_HIP_LIB; fi
  timeout -k 10 ${AB_BENCH_TIMEOUT:-180} python3 $root/bench.py --no-extras --no-cpu-baseline $AB_BENCH_ARGS 2>/dev/null |
    python3 -c "import sys,json; o=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('lib=$lib', o['value'], o['roofline']['frac'], o['roofline']['kernel_ms'])"
}
for i in $(seq 1 $rounds); do
  for lib in "$@"; do
    one "$lib" || { echo "lib=$lib round $i: bench process failed (status $?), stopping"; exit 1; }
  done
done
one "$1" || { echo "lib=$1 closing run: bench process failed (status $?), stopping"; exit 1; }
