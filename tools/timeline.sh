#!/bin/bash
# usage (GPU box): tools/timeline.sh <tag>  -> $OUT/timeline_<tag>.md : one training step's dispatches (rocprofv3 --kernel-trace)
tag=$1
R=$GRAFT_REPO_ROOT
export OUT=$(realpath -m "${OUT:-out}")                 # output directory (default: out/ of the repository)
cd /tmp; export TMPDIR=/tmp
timeout 200 rocprofv3 --kernel-trace -d $OUT/tl_$tag -o t -- python $R/bench.py --steps 6 --warmup 3 --no-cpu-baseline --no-ppo --no-fp32 --no-mlp --no-replay --no-x3 --no-dp-form --condition-ms 0 --no-box > $OUT/tl_$tag.log 2>&1
cd $R
python tools/rocpd_timeline.py $(find $OUT/tl_$tag -name "*.db" | head -1) > $OUT/timeline_$tag.md
rm -rf $OUT/tl_$tag
