#!/bin/bash
# Round profile (GPU box): bench line + rocprofv3 kernel stats + PMC HBM-traffic passes.
#   tools/profile_round.sh r01      -> $O/prof_r01*/ ; copy into profiles/ afterwards
set -o pipefail
tag=${1:-r01}
cd /tmp && export TMPDIR=/tmp && cd - > /dev/null
O=${BENCH_OUT:-bench_out}      # where the logs and JSON lines go
mkdir -p $O
B="bench.py --steps 300 --warmup 30 --no-cpu-baseline --no-roofline"
timeout -k 10 300 python3 bench.py --full > $O/bench_$tag.json 2> $O/bench_$tag.err || { echo bench failed; tail $O/bench_$tag.err; exit 1; }
echo "bench ok: $(cut -c1-200 $O/bench_$tag.json)"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_$tag -o run -- python3 $B > $O/prof_$tag.log 2>&1 || { echo trace failed; tail $O/prof_$tag.log; exit 1; }
echo trace ok
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/pmcf_$tag -o run -- python3 $B > $O/pmcf_$tag.log 2>&1 || { echo pmc fetch failed; tail $O/pmcf_$tag.log; exit 1; }
echo pmc fetch ok
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/pmcw_$tag -o run -- python3 $B > $O/pmcw_$tag.log 2>&1 || { echo pmc write failed; tail $O/pmcw_$tag.log; exit 1; }
echo pmc write ok
find $O/prof_$tag $O/pmcf_$tag $O/pmcw_$tag -name "*.csv" | head -20
