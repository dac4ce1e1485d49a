#!/bin/bash
# usage (on an MI355X): tools/pmc.sh <tag> [bench args...]  -> $PROF_OUT/<tag>_pmc_traffic.json
# two separate --pmc passes (FETCH_SIZE, WRITE_SIZE) of the same bench command, no trace domains
set -e
tag=$1; shift
R=${GRAFT_REPO_ROOT:-$(pwd)}
O=${PROF_OUT:-prof_out}; mkdir -p "$R/$O"       # output folder, under the repository root
cd /tmp && export TMPDIR=/tmp
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $R/$O/${tag}_fetch -- python3 $R/bench.py --no-cpu-baseline "$@" > $R/$O/${tag}_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $R/$O/${tag}_write -- python3 $R/bench.py --no-cpu-baseline "$@" > $R/$O/${tag}_write.log 2>&1
cd $R
python3 tools/pmc_traffic.py $O/${tag}_fetch $O/${tag}_write $O/${tag}_pmc_traffic.json > $O/${tag}_pmc_traffic.txt
rm -rf $O/${tag}_fetch $O/${tag}_write
# third pass: matrix-pipe busy cycles against the chip's active cycles (MFMA-busy fraction)
cd /tmp
rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $R/$O/${tag}_mfma -- python3 $R/bench.py --no-cpu-baseline "$@" > $R/$O/${tag}_mfma.log 2>&1 || true
cd $R
python3 tools/pmc_mfma.py $O/${tag}_mfma $O/${tag}_pmc_mfma.json ${PMC_CLOCK_MHZ:-} > $O/${tag}_pmc_mfma.txt || true
rm -rf $O/${tag}_mfma
