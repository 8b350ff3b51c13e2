#!/bin/bash
# usage: tools/kprof.sh <tag> <bench args...>  -- per-kernel average durations of a bench run (rocprofv3 kernel trace)
R=$GRAFT_REPO_ROOT; tag=$1; shift
OUT=${HTJ2K_PROF_OUT:-$R/build/prof}; mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/kprof_$tag -o bench -- python3 $R/bench.py "$@" > $OUT/kprof_$tag.log 2>&1
python3 - <<PY
import csv
print("== $tag", "$*")
for r in csv.DictReader(open("$OUT/kprof_$tag/bench_kernel_stats.csv")):
    if "rocclr" in r["Name"]: continue
    print("%-46s calls=%3s avg=%9.1f us  %5s%%" % (r["Name"].split("(")[0][:46], r["Calls"], float(r["AverageNs"])/1e3, r["Percentage"]))
PY
grep -a -o '"value": [0-9.]*' $OUT/kprof_$tag.log
