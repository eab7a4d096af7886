#!/bin/bash
# profile_glm.sh [OUT_DIR [OTHER_LIB]] -- on the GPU box: scripts/bench_glm.py's wall times, then the same calls alone under
# rocprofv3 twice -- once for the kernel times, once (a run of its own, on a 256 x 256 x 16 grid) for the fit kernel's issue
# counters -- merged into profiles/group_glm.json.  OUT_DIR receives the logs and the traces (default
# build/glm_profile, which git ignores).  With OTHER_LIB, a device library of another commit: frog_rank_add, frog_chain_sample
# and frog_chain_reslice, which share chain.hip with the new kernels, through OTHER_LIB and through the built library, three
# times each and in turn, so that the spread of a library against itself stands beside the difference between the two.
set -e -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT"
O=${1:-build/glm_profile}
mkdir -p $O/trace
timeout -k 10 500 python3 scripts/bench_glm.py --out $O/group_glm.json > $O/bench.log 2> $O/bench.err
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/trace -o p --output-format csv -- python3 scripts/bench_glm.py --trace-run > $O/trace.log 2>&1
timeout -k 10 300 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_SMEM SQ_INSTS_LDS SQ_ACTIVE_INST_VALU SQ_WAIT_INST_ANY \
    -d $O/trace/pmc -o p --output-format csv -- python3 scripts/bench_glm.py --trace-run --depth 16 > $O/pmc.log 2>&1
echo 16 > $O/trace/pmc_depth
if [ -n "$2" ]; then
  for lib in "$2" frog_amd/lib/libfrog_hip.so "$2" frog_amd/lib/libfrog_hip.so "$2" frog_amd/lib/libfrog_hip.so; do
    timeout -k 10 120 python3 scripts/bench_glm.py --ab "$lib" 2>> $O/ab.err | tail -1 >> $O/trace/ab.jsonl
  done
fi
python3 scripts/bench_glm.py --merge $O/trace --out $O/group_glm.json > /dev/null
cp $O/group_glm.json profiles/group_glm.json
cat profiles/group_glm.json
