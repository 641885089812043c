#!/bin/bash
# build/libv_<name>.so from the working tree, or from a git revision of the library sources (for tools/ab_round.sh).
# The library carries the hash of the sources it was compiled from (the Makefile's digest), so a variant built from
# another revision never reports the working tree's hash.
#   usage: bash tools/build_variant.sh <name> [revision]
set -e
NAME=$1; REV=${2:-}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
SRC=lcgp_amd/csrc/lcgp_hip.hip; HDR=include/lcgp_hip.h; SCHED=lcgp_amd/csrc/fill_sched.h
SUBSET=lcgp_amd/csrc/sobol_subset.h      # (absent from revisions before the subset pass: left out of their digest, as it was then)
T=$(mktemp -d); trap 'rm -rf "$T"' EXIT
mkdir -p $ROOT/build $T/lcgp_amd/csrc $T/include
[ -z "$REV" ] || git -C $ROOT cat-file -e $REV:$SUBSET 2>/dev/null || SUBSET=
for f in $SRC $HDR $SCHED $SUBSET; do
  if [ -z "$REV" ]; then cp $ROOT/$f $T/$f; else git -C $ROOT show $REV:$f > $T/$f; fi
done
HASH=$(cd $T && cat $SRC $HDR $SCHED $SUBSET | sha256sum | cut -c1-16)
hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -shared "-DLCGP_SRC_HASH=\"LCGP_SRC_HASH=$HASH\"" -o $ROOT/build/libv_$NAME.so $T/$SRC
echo built build/libv_$NAME.so "(source hash $HASH)"
