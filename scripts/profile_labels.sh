#!/bin/bash
# profile_labels.sh [OUT_DIR] -- on the GPU box: scripts/bench_labels.py's wall times and bin/FuseLabels' phase lines, then one
# accumulation alone under rocprofv3 for the kernel times, merged into profiles/label_fusion.json.  OUT_DIR
# receives the logs and the trace (default build/labels_profile, which git ignores).
set -e -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT"
O=${1:-build/labels_profile}
mkdir -p $O
timeout -k 10 500 python3 scripts/bench_labels.py --out $O/label_fusion.json > $O/bench.log 2> $O/bench.err
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/trace -o p --output-format csv -- python3 scripts/bench_labels.py --trace-run > $O/trace.log 2>&1
python3 scripts/bench_labels.py --merge $O/trace --out $O/label_fusion.json > /dev/null
cp $O/label_fusion.json profiles/label_fusion.json
cat profiles/label_fusion.json
