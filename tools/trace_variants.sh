#!/bin/bash
# per-kernel sums of one evaluation for several builds (build/libv_<name>.so, loaded through LCGP_HIP_LIB; the product
# library is never touched): bash tools/trace_variants.sh <tag> <q> name1 name2 ...
# Stops at the first trace that fails or times out.
set -e
TAG=$1; Q=$2; shift; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
export TMPDIR=/tmp
for v in "$@"; do test -f $ROOT/build/libv_$v.so || { echo "missing build/libv_$v.so" >&2; exit 1; }; done
for v in "$@"; do
  rm -rf /tmp/tr_$v
  (cd /tmp && LCGP_HIP_LIB=$ROOT/build/libv_$v.so timeout -k 10 600 rocprofv3 --kernel-trace --output-format csv -d /tmp/tr_$v -- python3 $ROOT/tools/run_evals.py 3 $Q 4 > /tmp/tr_$v.log 2>&1)
  F=$(find /tmp/tr_$v -name '*kernel_trace.csv' | head -1)
  python tools/trace_view.py $F > gpurun_out/trace_${TAG}_$v.txt
  echo "== $v"; sed -n '/--- last evaluation/,$p' gpurun_out/trace_${TAG}_$v.txt | head -14
done
