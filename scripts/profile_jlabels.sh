#!/bin/bash
# profile_jlabels.sh [OUT_DIR [OTHER_LIB [DEPTH]]] -- on the GPU box: scripts/bench_jlabels.py's wall times on the 256 x 256 x DEPTH
# grid (default 256), then one accumulation under rocprofv3 twice -- once for the kernel times, once (a run of its own, on a
# 256 x 256 x 16 grid) for the solve kernel's LDS and issue counters -- then bin/AtlasSegment with -j 1 and without, merged into
# profiles/joint_fusion.json.  OUT_DIR receives the logs and the traces (default build/jlabels_profile, which
# git ignores).  With OTHER_LIB, a device library of another commit: frog_labels_add, frog_wlabels_add and frog_chain_reslice,
# which share chain.hip with the new kernel, through OTHER_LIB and through the built library, twice each and in turn, so that
# the spread of a library against itself stands beside the difference between the two.
set -e -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT"
O=${1:-build/jlabels_profile}
DEPTH=${3:-256}
mkdir -p $O/trace
timeout -k 10 600 python3 scripts/bench_jlabels.py --depth $DEPTH --out $O/joint_fusion.json > $O/bench.log 2> $O/bench.err
timeout -k 10 600 rocprofv3 --kernel-trace -d $O/trace -o p --output-format csv -- python3 scripts/bench_jlabels.py --trace-run --depth $DEPTH > $O/trace.log 2>&1
echo $DEPTH > $O/trace/trace_depth
timeout -k 10 300 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_LDS SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_WAIT_INST_LDS \
    -d $O/trace/pmc -o p --output-format csv -- python3 scripts/bench_jlabels.py --trace-run --depth 16 > $O/pmc.log 2>&1
echo 16 > $O/trace/pmc_depth
if [ -n "$2" ]; then
  for lib in "$2" frog_amd/lib/libfrog_hip.so "$2" frog_amd/lib/libfrog_hip.so; do
    timeout -k 10 120 python3 scripts/bench_jlabels.py --ab "$lib" 2>> $O/ab.err | tail -1 >> $O/trace/ab.jsonl
  done
fi
timeout -k 10 900 python3 scripts/bench_jlabels.py --tool --depth $DEPTH 2> $O/tool.err | tail -1 > $O/trace/tool.json
python3 scripts/bench_jlabels.py --merge $O/trace --out $O/joint_fusion.json > /dev/null
cp $O/joint_fusion.json profiles/joint_fusion.json
cat profiles/joint_fusion.json
