#!/bin/bash
# Diagnostic library variants (same sources, different -D switches) into build/,
# built as the library itself is (__graft_entry__.build: its source list and flags).
# usage: tools/build_variants.sh NAME "-DFLAG=.. -DFLAG2=.." [NAME2 "FLAGS2" ...]
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$R/build"
while [ $# -ge 2 ]; do
  (cd "$R" && python -c 'import shlex, sys, __graft_entry__ as g
g.build(extra=shlex.split(sys.argv[2]), out=sys.argv[1])' "$R/build/libmfgp_$1.so" "$2") &
  shift 2
done
wait
ls -la "$R/build"
