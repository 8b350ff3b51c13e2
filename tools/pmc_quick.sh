#!/bin/bash
# usage: tools/pmc_quick.sh <tag> <counter> -- one PMC pass of the one-job bench, per-kernel means (A/B of a single counter)
R=$GRAFT_REPO_ROOT; tag=$1; ctr=$2
OUT=${HTJ2K_PROF_OUT:-$R/build/prof}; mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --pmc $ctr --output-format csv -d $OUT/pmcq_$tag -o b -- python3 $R/bench.py --steps 3 --warmup 1 --jobs 1 > $OUT/pmcq_$tag.log 2>&1 || { tail -3 $OUT/pmcq_$tag.log; exit 1; }
python3 $R/tools/pmc_summary.py $OUT/pmcq_$tag/b_counter_collection.csv | grep "k_ht_\|k_idwt"
