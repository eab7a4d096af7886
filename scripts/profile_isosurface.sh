#!/bin/bash
# profile_isosurface.sh [OUT_DIR] -- on the GPU box: scripts/bench_isosurface.py's wall times, then the same calls alone under
# rocprofv3 for the kernel times, merged with each kernel's bytes at the HBM rate into profiles/isosurface.json.
# OUT_DIR receives the logs and the trace (default build/isosurface_profile, which git ignores).
set -e -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT"
O=${1:-build/isosurface_profile}
mkdir -p $O/trace
timeout -k 10 400 python3 scripts/bench_isosurface.py --out $O/isosurface.json > $O/bench.log 2> $O/bench.err
timeout -k 10 200 rocprofv3 --kernel-trace --stats -d $O/trace -o p --output-format csv -- python3 scripts/bench_isosurface.py --trace-run > $O/trace.log 2>&1
python3 scripts/bench_isosurface.py --merge $O/trace --out $O/isosurface.json > /dev/null
cp $O/isosurface.json profiles/isosurface.json
cat profiles/isosurface.json
