#!/bin/bash
# profile_smooth.sh [OUT_DIR [OTHER_LIB]] -- on the GPU box: scripts/bench_smooth.py's wall times, then smoothed adds alone under
# rocprofv3 for the kernel times, merged into profiles/group_smooth.json.  OUT_DIR receives the logs and the
# trace (default build/smooth_profile, which git ignores).  With OTHER_LIB, a device library of another commit:
# frog_glm_add_jacobian without smoothing and frog_glm_permute, which share chain.hip with the new kernels, through OTHER_LIB
# and through the built library, three times each and in turn, so that the spread of a library against itself stands beside
# the difference between the two.
set -e -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT"
O=${1:-build/smooth_profile}
mkdir -p $O/trace
timeout -k 10 500 python3 scripts/bench_smooth.py --out $O/group_smooth.json > $O/bench.log 2> $O/bench.err
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/trace -o p --output-format csv -- python3 scripts/bench_smooth.py --trace-run > $O/trace.log 2>&1
python3 scripts/bench_smooth.py --merge-trace $O/trace --out $O/group_smooth.json > /dev/null
if [ -n "$2" ]; then
  for lib in "$2" frog_amd/lib/libfrog_hip.so "$2" frog_amd/lib/libfrog_hip.so "$2" frog_amd/lib/libfrog_hip.so; do
    timeout -k 10 120 python3 scripts/bench_smooth.py --ab "$lib" 2>> $O/ab.err | tail -1 >> $O/ab.jsonl
  done
  python3 scripts/bench_smooth.py --merge $O/ab.jsonl --out $O/group_smooth.json > /dev/null
fi
cp $O/group_smooth.json profiles/group_smooth.json
cat profiles/group_smooth.json
