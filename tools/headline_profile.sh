#!/bin/bash
# GPU box: the headline bench line, its rocprofv3 kernel-trace summary and the
# HBM-traffic PMC passes (FETCH_SIZE, WRITE_SIZE in separate runs), for profiles/.
# usage: [OUT=dir] tools/headline_profile.sh TAG     (OUT: where the results go, default profile_out)
set -o pipefail
TAG=${1:-r02}
OUT=${OUT:-profile_out}
export TMPDIR=/tmp
mkdir -p $OUT
B="--full --extra= --cpu-baseline 0 --steps 3"
timeout -k 10 420 python3 -u bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err || exit 1
echo "bench done"
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_kt -o run -- python3 bench.py $B > $OUT/${TAG}_kt.log 2>&1 || exit 1
cp "$(find $OUT/${TAG}_kt -name "*kernel_stats.csv" -print -quit)" $OUT/${TAG}_cfg2_kernel_stats.csv || exit 1
echo "kernel trace done"
timeout -s KILL 240 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/${TAG}_pf -o run -- python3 bench.py $B > $OUT/${TAG}_pf.log 2>&1 || exit 1
timeout -s KILL 240 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/${TAG}_pw -o run -- python3 bench.py $B > $OUT/${TAG}_pw.log 2>&1 || exit 1
python3 tools/pmc_traffic.py $OUT/${TAG}_pf $OUT/${TAG}_pw "" > $OUT/${TAG}_cfg2_pmc_traffic.json || exit 1
echo "pmc done"
head -c 400 $OUT/${TAG}_bench.json
