#!/bin/bash
# usage (GPU box): tools/pmc_pass.sh <tag> "<counters...>"  -> $OUT/pmc_<tag>.md  (one rocprofv3 --pmc pass of a short bench run)
tag=$1; shift
R=$GRAFT_REPO_ROOT
export OUT=$(realpath -m "${OUT:-out}")                 # output directory (default: out/ of the repository)
cd /tmp; export TMPDIR=/tmp
timeout 150 rocprofv3 --pmc $@ -d $OUT/pmc_$tag -o p -- python $R/bench.py --steps 2 --warmup 3 --no-cpu-baseline --no-ppo --no-fp32 --no-mlp --no-replay --no-x3 --no-dp-form --condition-ms 0 --no-box > $OUT/pmc_$tag.log 2>&1
cd $R
python tools/rocpd_pmc_summary.py $(find $OUT/pmc_$tag -name "*.db" | head -1) > $OUT/pmc_$tag.md 2>> $OUT/pmc_$tag.log
rm -rf $OUT/pmc_$tag
