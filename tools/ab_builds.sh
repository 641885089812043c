#!/bin/bash
# Same-box A/B of two or more BUILDS of the library (timing differs by +-1.5 % between boxes of the pool, so builds are
# compared by alternating them in one run on one box).
#   usage: bash tools/ab_builds.sh "<tools/ab.py arguments>" name1 name2 ...      with the builds at build/libv_<name>.so
# Each run loads its build through LCGP_HIP_LIB; the product library is never touched.  Results should be checked for
# equality first (tools/ab_round.sh; tools/dump_eval.py writes NLL + gradient of three configurations to an .npy).
# Stops at the first run that fails or times out.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
ARGS=$1; shift
for v in "$@"; do test -f $ROOT/build/libv_$v.so || { echo "missing build/libv_$v.so" >&2; exit 1; }; done
for rep in 1 2; do
  for v in "$@"; do
    echo "== $v"
    LCGP_HIP_LIB=$ROOT/build/libv_$v.so timeout -k 10 600 python $ROOT/tools/ab.py $ARGS "d:"
  done
done
