#!/bin/bash
# profile_rank.sh [OUT_DIR] -- on the GPU box: scripts/bench_rank.py's wall times, then the same calls alone under rocprofv3 for
# the kernel times, merged into profiles/rank.json.  OUT_DIR receives the logs and the trace (default
# build/rank_profile, which git ignores).
set -e -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT"
O=${1:-build/rank_profile}
mkdir -p $O
timeout -k 10 500 python3 scripts/bench_rank.py --out $O/rank.json > $O/bench.log 2> $O/bench.err
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/trace -o p --output-format csv -- python3 scripts/bench_rank.py --trace-run > $O/trace.log 2>&1
python3 scripts/bench_rank.py --merge $O/trace --out $O/rank.json > /dev/null
cp $O/rank.json profiles/rank.json
cat profiles/rank.json
