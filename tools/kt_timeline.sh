#!/bin/bash
# rocprofv3 kernel trace of a short bench run per config, then the per-kernel averages and launch gaps.
# Traces and logs go under OUT (default: build/kt_timeline in the repository).
set -o pipefail
R="${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}"
OUT=${OUT:-$R/build/kt_timeline}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
for c in ${CFGS:-c3 c2}; do
  timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d $OUT/kt_$c -o kt -- python3 $R/bench.py --full --config $c --steps 2 --warmup 1 --no-cpu-baseline --no-hbm-roofline > $OUT/kt_$c.log 2>&1 || exit 1
  echo "== $c"; python3 $R/tools/kt_gaps.py $OUT/kt_$c --last ${LAST:-600} || exit 1
done
