#!/bin/bash
# GPU-box check: parity tests, the C2 bench line and the acting-loop bench.  Usage: tools/gpu_check2.sh TAG
set -o pipefail
tag=${1:-run}
O=${BENCH_OUT:-bench_out}      # where the logs and JSON lines go
mkdir -p $O
timeout -k 10 300 python3 -m pytest tests -m gpu -x -q > $O/pytest_$tag.log 2>&1
rc=$?; tail -3 $O/pytest_$tag.log; echo "pytest rc=$rc"
[ $rc -ne 0 ] && exit $rc
timeout -k 10 300 python3 bench.py --full --no-cpu-baseline > $O/bench_$tag.json 2> $O/bench_$tag.err || { tail -20 $O/bench_$tag.err; exit 1; }
timeout -k 10 300 python3 bench_loop.py > $O/loop_$tag.json 2> $O/loop_$tag.err || { tail -20 $O/loop_$tag.err; exit 1; }
python3 - "$O/bench_$tag.json" "$O/loop_$tag.json" <<'PY'
import json, sys
for f in sys.argv[1:]:
    d = json.loads(open(f).read().strip().splitlines()[-1])
    print(f, d["value"], d.get("roofline", {}).get("frac"), d.get("serial_value"))
PY
