#!/bin/bash
# profile_field.sh [BASELINE_LIB [OUT_DIR]] -- on the GPU box: scripts/bench_field.py's wall times, then the same calls alone
# under rocprofv3 for the kernel times, merged into profiles/field_sample.json.  BASELINE_LIB: another build of
# libfrog_hip.so (e.g. the parent commit's; "" for none) whose check and reslice are timed in turn with this one's.  OUT_DIR
# receives the logs and the trace (default build/field_profile, which git ignores).
set -e -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT"
O=${2:-build/field_profile}
mkdir -p $O
timeout -k 10 400 python3 scripts/bench_field.py --out $O/field_sample.json ${1:+--baseline-lib "$1"} > $O/bench.log 2> $O/bench.err
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/trace -o p --output-format csv -- python3 scripts/bench_field.py --trace-run > $O/trace.log 2>&1
python3 scripts/bench_field.py --merge $O/trace --out $O/field_sample.json > /dev/null
cp $O/field_sample.json profiles/field_sample.json
cat profiles/field_sample.json
