#!/bin/bash
# profile_surface.sh [OUT_DIR] -- on the GPU box: scripts/bench_surface.py's wall times (frog_surface_add beside frog_labels_add,
# the create, a whole-grid distance map, bin/FuseLabels without and with -d 1), then one create and one add per image alone
# under rocprofv3 for the kernel times of the three passes with and without cropping, merged into profiles/surface.json
# (DESIGN.md 21).  OUT_DIR receives the logs and the trace (default build/surface_profile, which git ignores).
set -e -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT"
O=${1:-build/surface_profile}
mkdir -p $O
TRACE="rocprofv3 --kernel-trace --stats -o p --output-format csv"
timeout -k 10 900 python3 scripts/bench_surface.py --out $O/surface.json > $O/bench.log 2> $O/bench.err
timeout -k 10 400 $TRACE -d $O/trace -- python3 scripts/bench_surface.py --trace-run > $O/trace.log 2>&1
python3 scripts/bench_surface.py --merge $O/trace --out $O/surface.json > /dev/null
cp $O/surface.json profiles/surface.json
cat profiles/surface.json
