#!/bin/bash
# profile_modes.sh [OUT_DIR] -- on the GPU box: scripts/bench_modes.py's wall times, then the same calls alone under rocprofv3 for
# the kernel times, merged with the two yardsticks (the stored bytes at the HBM rate, the products and sums at the f64 rate) into
# profiles/group_modes.json.  OUT_DIR receives the logs and the trace (default build/modes_profile, which git
# ignores).
set -e -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT"
O=${1:-build/modes_profile}
mkdir -p $O/trace
timeout -k 10 900 python3 scripts/bench_modes.py --out $O/group_modes.json > $O/bench.log 2> $O/bench.err
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/trace -o p --output-format csv -- python3 scripts/bench_modes.py --trace-run > $O/trace.log 2>&1
python3 scripts/bench_modes.py --merge $O/trace --out $O/group_modes.json > /dev/null
cp $O/group_modes.json profiles/group_modes.json
cat profiles/group_modes.json
