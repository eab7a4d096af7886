#!/bin/bash
# profile_staple.sh [OUT_DIR] -- on the GPU box: scripts/bench_staple.py's wall times, then one accumulation and a solve of five
# M-steps alone under rocprofv3 for the per-iteration kernel times of the E-step and the M-step, merged into
# profiles/staple.json.  Where frog_amd/lib/variants/libfrog_hip_staple_perlane.so exists
# (scripts/build_variant.sh staple_perlane -DSTAPLE_MSTEP_UNIFORM=0) the same run is traced with it in the same session: the A/B
# of the M-step with and without the wave-uniform shortcut.  OUT_DIR receives the logs and the traces (default
# build/staple_profile, which git ignores).
set -e -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT"
O=${1:-build/staple_profile}
mkdir -p $O
TRACE="rocprofv3 --kernel-trace --stats -o p --output-format csv"
timeout -k 10 500 python3 scripts/bench_staple.py --out $O/staple.json > $O/bench.log 2> $O/bench.err
timeout -k 10 300 $TRACE -d $O/trace -- python3 scripts/bench_staple.py --trace-run > $O/trace.log 2>&1
python3 scripts/bench_staple.py --merge $O/trace --out $O/staple.json > /dev/null
if [ -f frog_amd/lib/variants/libfrog_hip_staple_perlane.so ]; then
  python3 scripts/bench_staple.py --merge $O/trace --arm uniform --out $O/staple.json > /dev/null
  FROG_HIP_LIB=variants/libfrog_hip_staple_perlane.so timeout -k 10 300 $TRACE -d $O/trace_perlane -- python3 scripts/bench_staple.py --trace-run > $O/trace_perlane.log 2>&1
  python3 scripts/bench_staple.py --merge $O/trace_perlane --arm per_lane --out $O/staple.json > /dev/null
fi
cp $O/staple.json profiles/staple.json
cat profiles/staple.json
