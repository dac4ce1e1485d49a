#!/bin/bash
# usage (on the GPU box): tools/prof.sh <tag> [bench args...]
# rocprofv3 kernel trace + stats of bench.py; summary -> $PROF_OUT/<tag>.txt, CSV kept as
# $PROF_OUT/<tag>_kernel_stats.csv, bench JSON line -> $PROF_OUT/<tag>.json
set -e
tag=$1; shift
R=${GRAFT_REPO_ROOT:-$(pwd)}
O=${PROF_OUT:-prof_out}; mkdir -p "$R/$O"       # output folder, under the repository root
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $R/$O/$tag -- python3 $R/bench.py --no-cpu-baseline "$@" > $R/$O/$tag.log 2>&1
cd $R
grep '^{"metric"' $O/$tag.log > $O/$tag.json || true
steps=$(python3 -c "import json;d=json.load(open('$O/$tag.json'));print(d['steps']+d['warmup']+1)")
python3 tools/prof_summary.py $O/$tag $steps 30 $O/${tag}_buckets.json > $O/$tag.txt
cp $(find $O/$tag -name '*kernel_stats.csv' | head -1) $O/${tag}_kernel_stats.csv
rm -rf $O/$tag
