#!/bin/bash
# profile_wlabels.sh [OUT_DIR [OTHER_LIB]] -- on the GPU box: scripts/bench_wlabels.py's wall times, then the target and three adds at radius
# 1, 2 and 4 under rocprofv3 twice -- once for the kernel times, once (a run of its own) for the vote kernel's LDS and issue
# counters -- merged into profiles/weighted_fusion.json.  OUT_DIR receives the logs and the traces (default
# build/wlabels_profile, which git ignores).  With OTHER_LIB, a device library of another commit: frog_labels_add and
# frog_chain_reslice, which share chain.hip with the new kernels, through OTHER_LIB and through the built library, twice each
# and in turn, so that the spread of a library against itself stands beside the difference between the two.
set -e -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT"
O=${1:-build/wlabels_profile}
mkdir -p $O
timeout -k 10 400 python3 scripts/bench_wlabels.py --out $O/weighted_fusion.json > $O/bench.log 2> $O/bench.err
timeout -k 10 300 rocprofv3 --kernel-trace -d $O/trace -o p --output-format csv -- python3 scripts/bench_wlabels.py --trace-run > $O/trace.log 2>&1
timeout -k 10 300 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_LDS SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAIT_INST_LDS \
    -d $O/trace/pmc -o p --output-format csv -- python3 scripts/bench_wlabels.py --trace-run > $O/pmc.log 2>&1
if [ -n "$2" ]; then
  for lib in "$2" frog_amd/lib/libfrog_hip.so "$2" frog_amd/lib/libfrog_hip.so; do
    timeout -k 10 120 python3 scripts/bench_wlabels.py --ab "$lib" 2>> $O/ab.err | tail -1 >> $O/trace/ab.jsonl
  done
fi
python3 scripts/bench_wlabels.py --merge $O/trace --out $O/weighted_fusion.json > /dev/null
cp $O/weighted_fusion.json profiles/weighted_fusion.json
cat profiles/weighted_fusion.json
