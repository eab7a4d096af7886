#!/usr/bin/env python3
"""Threshold-free cluster enhancement at volume size: scripts/bench_clusters.py's case -- the 256^3 grid, 20
images, a 3-column design, one contrast, permutations of the group column, connectivity 26 -- with dh 0.1, E 0.5, H 2, on the
registered group of scripts/bench_glm.py and on white noise.

  bench_tfce.py [--out FILE] [--perms N]  wall times (host clock around whole calls; every call ends in a synchronisation):
                                   frog_glm_permute and frog_glm_permute_tfce, frog_tfce_finish over the slots, one
                                   frog_tfce_map; the highest levels and the set voxels per level of some slots;
                                   bin/GroupStats end to end with 100 permutations, with and without -tf 1
  bench_tfce.py --trace-run        frog_tfce_finish of 64 slots of the noise group, nothing else after the fill: the command to
                                   run under `rocprofv3 --kernel-trace --stats -d DIR -o p --output-format csv`
  bench_tfce.py --merge-trace DIR  reads DIR's kernel trace (no device needed) and adds the kernel times of the finish
  bench_tfce.py --ab LIB           frog_glm_permute (64 permutations, the median of 9 calls) through the device library LIB
                                   (a build of another commit, which need not export frog_tfce_*): one JSON line
  bench_tfce.py --merge FILE       adds FILE's --ab lines (no device needed) to the output file"""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_glm import IMAGES, DISTINCT, filled              # noqa: E402
from bench_labels import GRID, N, chain_links, stats, timed  # noqa: E402
import bench_clusters                                        # noqa: E402

DH, E, H, CONNECTIVITY = 0.1, 0.5, 2, 26
CONTRAST = [[0.0, 1.0, 0.0]]
NEW_SYMBOLS = ("frog_tfce_", "frog_glm_permute_tfce")
FINISH_KERNELS = ("tfce_top_kernel", "tfce_mask_kernel", "ccl_init_kernel", "ccl_link_kernel", "ccl_count_kernel", "tfce_accumulate_kernel",
                  "tfce_round_kernel")
SAMPLED = (0, 1, 2, 3)


def noise_group():
    from bench_glm import design
    from frog_amd.volume import GroupGLM
    rng = np.random.default_rng(24)
    acc = GroupGLM(GRID, design())
    for _ in range(IMAGES):
        acc.add(rng.standard_normal((N, N, N), np.float32))
    return acc


def one_group(acc, perm, repeats):
    """permute beside permute_tfce, finish and one map through `acc`."""
    from frog_amd.volume import TfceSink
    perms = len(perm)
    out = {}
    acc.permute(CONTRAST, perm[:64], None, [1])              # the first launches of a process
    plain = [timed(lambda: acc.permute(CONTRAST, perm, None, [1])) for _ in range(repeats)]
    out["glm_permute"] = dict(stats([t for _, t in plain]), per_permutation_ms=round(float(np.median([t for _, t in plain])) / perms, 4))
    t_fill, t_finish, t_create = [], [], []
    for r in range(repeats):
        sink, ms = timed(lambda: TfceSink(GRID, perms, 1, DH, E, H, False, CONNECTIVITY))
        t_create.append(ms)
        got, ms = timed(lambda: acc.permute_tfce(sink, CONTRAST, perm, None, [1]))
        t_fill.append(ms)
        assert got[0].tobytes() == plain[0][0][0].tobytes() and got[1].tobytes() == plain[0][0][1].tobytes()
        best, ms = timed(sink.finish)
        t_finish.append(ms)
        if r + 1 < repeats:
            sink.close()
    out["tfce_create"] = stats(t_create)
    out["glm_permute_tfce"] = dict(stats(t_fill), per_permutation_ms=round(float(np.median(t_fill)) / perms, 4))
    out["tfce_finish"] = dict(stats(t_finish), slots=perms, per_slot_ms=round(float(np.median(t_finish)) / perms, 4))
    _, ms = timed(lambda: sink.map(1, 0))
    out["tfce_map_slot_1"] = {"ms": round(ms, 3)}
    levels = {k: np.bincount(sink.levels(k, 0).reshape(-1), minlength=256) for k in SAMPLED if k < perms}
    out["highest_level_of_slots_%s" % "_".join(str(k) for k in levels)] = [int(np.flatnonzero(c).max()) for c in levels.values()]
    above = np.cumsum(levels[1][::-1])[::-1]                # voxels with level >= k
    out["set_voxels_per_level_of_slot_1"] = {str(k): int(above[k]) for k in range(1, 256) if above[k]}
    out["set_voxels_of_all_levels_of_slot_1_in_grids"] = round(float(above[1:].sum()) / N ** 3, 3)
    out["max_tfce"] = {"observed": float(best[0, 0, 0]), "null_median": float(np.median(best[1:, 0, 0])), "null_max": float(best[1:, 0, 0].max())}
    sink.close()
    return out


def measure(args):
    from frog_amd.chain import Chain, invert
    from frog_amd.volume import glm_draw
    perm, _ = glm_draw(IMAGES, args.perms, 1)
    out = {"what": "scripts/bench_tfce.py on one MI355X: scripts/bench_glm.py's group (%d images, 256^3 grid, 3 columns, one contrast), %d "
                   "permutations of the group column, dh %.1f, E %.1f, H %d, connectivity %d, one-sided; wall times are host-clock times of "
                   "whole calls, copies included" % (IMAGES, args.perms, DH, E, H, CONNECTIVITY),
           "voxels": N ** 3, "permutations": args.perms}
    acc = filled([Chain(invert(chain_links(100 + i))) for i in range(DISTINCT)])
    out["group"] = one_group(acc, perm, args.repeats)
    acc.close()
    acc = noise_group()
    out["noise"] = dict(what="%d volumes of white N(0, 1) noise on the grid, the same design and permutations" % IMAGES, **one_group(acc, perm, args.repeats))
    acc.close()
    out["slots_per_launch"] = min(args.perms, 64)
    words = (N ** 3 + 31) // 32
    out["device_bytes"] = {"levels": args.perms * words * 32, "workspace_per_slot_of_a_launch": 16 * N ** 3 + 4 * words}
    if not args.no_tool:
        out["tool"] = {"without_tf": tool(False), "with_tf": tool(True)}
    return out


def tool(enhance):
    """bin/GroupStats on bench_glm's files with 100 permutations (bench_clusters.tool's files and phases)."""
    return bench_clusters.tool(False, ["-tf", "1", "-cc", str(CONNECTIVITY)] if enhance else [])


def trace_run(args):
    from frog_amd.volume import TfceSink, glm_draw
    perm, _ = glm_draw(IMAGES, 64, 1)
    acc = noise_group()
    sink = TfceSink(GRID, 64, 1, DH, E, H, False, CONNECTIVITY)
    acc.permute_tfce(sink, CONTRAST, perm, None, [1])
    best = sink.finish()
    print(json.dumps({"slots": 64, "max_tfce_median": float(np.median(best))}))
    sink.close()
    acc.close()


def merge_trace(args, out):
    rows = []
    for f in glob.glob(os.path.join(args.merge_trace, "**", "*kernel_stats.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    table = {}
    for r in rows:
        name = next((k for k in FINISH_KERNELS if k in r["Name"]), None)
        if name:
            e = table.setdefault(name, {"launches": 0, "total_ms": 0.0})
            e["launches"] += int(r["Calls"])
            e["total_ms"] += float(r["TotalDurationNs"]) / 1e6
    for e in table.values():
        e["total_ms"] = round(e["total_ms"], 3)
        e["per_slot_ms"] = round(e["total_ms"] / 64, 4)
    out["finish_of_64_noise_slots_by_kernel_under_rocprofv3"] = table


def ab(args):
    """frog_glm_permute, which existed before frog_tfce, through another build of the device library."""
    os.environ["FROG_HIP_LIB"] = os.path.abspath(args.ab)
    from frog_amd import _abi
    _abi.HIP_SYMBOLS = {k: v for k, v in _abi.HIP_SYMBOLS.items() if not k.startswith(NEW_SYMBOLS)}
    from frog_amd.chain import Chain, invert
    from frog_amd.volume import glm_draw
    acc = filled([Chain(invert(chain_links(100 + i))) for i in range(DISTINCT)])
    perm, _ = glm_draw(IMAGES, 64, 1)
    t = [timed(lambda: acc.permute(CONTRAST, perm, None, [1]))[1] for _ in range(10)][1:]
    acc.close()
    print(json.dumps({"library": args.ab, "glm_permute_64": stats(t)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_tfce.json"))
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--perms", type=int, default=1000)
    ap.add_argument("--no-tool", action="store_true")
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--merge-trace")
    ap.add_argument("--ab")
    ap.add_argument("--merge")
    args = ap.parse_args()
    if args.ab:
        return ab(args)
    if args.trace_run:
        return trace_run(args)
    if args.merge or args.merge_trace:
        out = json.load(open(args.out))
        if args.merge:
            out["glm_permute_by_library_in_turn"] = [json.loads(line) for line in open(args.merge) if line.strip().startswith("{")]
        if args.merge_trace:
            merge_trace(args, out)
    else:
        out = measure(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
