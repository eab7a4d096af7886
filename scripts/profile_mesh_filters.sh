#!/bin/bash
# profile_mesh_filters.sh [OUT_DIR] -- on the GPU box: scripts/bench_mesh_filters.py's wall times, then the same calls alone under
# rocprofv3 for the kernel times, merged with the pass kernel's bytes at the HBM rate into profiles/mesh_filters.json.
# OUT_DIR receives the logs and the trace (default build/mesh_filters_profile, which git ignores).
set -e -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT"
O=${1:-build/mesh_filters_profile}
mkdir -p $O/trace16 $O/trace12
timeout -k 10 400 python3 scripts/bench_mesh_filters.py --out $O/mesh_filters.json > $O/bench.log 2> $O/bench.err
FROG_MESH_STRIDE=4 timeout -k 10 200 rocprofv3 --kernel-trace --stats -d $O/trace16 -o p --output-format csv -- python3 scripts/bench_mesh_filters.py --trace-run > $O/trace16.log 2>&1
FROG_MESH_STRIDE=3 timeout -k 10 200 rocprofv3 --kernel-trace --stats -d $O/trace12 -o p --output-format csv -- python3 scripts/bench_mesh_filters.py --trace-run > $O/trace12.log 2>&1
python3 scripts/bench_mesh_filters.py --merge $O/trace16 --key kernels_under_rocprofv3_rows_of_16_bytes --out $O/mesh_filters.json > /dev/null
python3 scripts/bench_mesh_filters.py --merge $O/trace12 --key kernels_under_rocprofv3_rows_of_12_bytes --out $O/mesh_filters.json > /dev/null
cp $O/mesh_filters.json profiles/mesh_filters.json
cat profiles/mesh_filters.json
