#!/usr/bin/env python3
"""frog_staple at volume size: scripts/bench_labels.py's case -- a 256^3 grid, 20 uint16 label images with 20
RadLex-like values in blocks, one seeded 1 + 7 link chain per image.

  bench_staple.py [--out FILE]        wall times (host clock around whole calls, each of which ends in a synchronisation or a
                                      device-to-host copy): per add, finish, solve (restrict 0 and 1), fused; and the ratio
                                      of one solve to the 20 adds before it
  bench_staple.py --trace-run         one accumulation and one solve of --iterations M-steps (tol 0), nothing else: the
                                      command to run under `rocprofv3 --kernel-trace --stats -d DIR -o p --output-format csv`
  bench_staple.py --merge DIR [--arm NAME]
                                      reads DIR's kernel trace (no device needed) and adds the per-launch kernel times, the
                                      bytes each kernel moves by the count below and the share of 8 TB/s that makes; NAME
                                      files them under "ab" (the M-step with and without the wave-uniform shortcut)
Bytes by count, A active voxels of V, n images, L labels: the E-step reads n bytes of D and writes 4 L bytes of q per active
voxel and reads the mask; the M-step reads, per image tile, 4 L bytes of q per active voxel and the mask, and n bytes of D per
active voxel over all tiles.  theta, S and the prior stay in the caches."""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_labels import GRID, N, PEAK_BYTES_PER_S, VALUES, chain_links, label_volume, stats, timed  # noqa: E402

ACC_WORDS = 6144                                            # STAPLE_ACC_WORDS (k_staple.hip.h)


def image_tiles(n, L):
    lw = min(L, 64, ACC_WORDS // L)
    it = max(1, min(n, ACC_WORDS // (L * lw)))
    return -(-n // it), -(-L // lw)


def moved(kind, n, L, V, A):
    if kind == "estep":
        return A * (n + 4 * L) + V
    tiles_i, tiles_l = image_tiles(n, L)
    return tiles_i * (4 * L * A + tiles_l * V) + tiles_l * n * A


def accumulate(n):
    from frog_amd.chain import Chain, invert
    from frog_amd.volume import Staple
    acc = Staple(GRID, n)
    times = []
    for i in range(n):
        v, c = (label_volume(i), GRID[1], GRID[2]), Chain(invert(chain_links(100 + i)))
        times.append(timed(lambda: acc.add(v, c, 0.0))[1])
        c.close()
    return acc, times


def measure(args):
    n = args.images
    out = {"what": "scripts/bench_staple.py on one MI355X: %d uint16 label images of 256^3 voxels with %d values, each through the "
                   "inverse of 1 matrix + 7 lattices onto a 256^3 grid at 400/256 mm; wall times are host-clock times of whole "
                   "calls, copies included" % (n, len(VALUES)),
           "images": n, "voxels": N ** 3, "wall": {}}
    w = out["wall"]
    t_add, t_adds, t_finish, t_fused = [], [], [], []
    t_solve = {False: [], True: []}
    for rep in range(args.repeats + 1):                     # the first round warms up
        acc, ta = accumulate(n)
        L, ms_finish = timed(acc.finish)
        for restrict in (False, True):
            (it, change, active), ms = timed(lambda: acc.solve(restrict=restrict))
            if rep:
                t_solve[restrict].append(ms)
            out["solve_restrict_%d" % restrict] = {"iterations": it, "change": change, "active_voxels": active}
        (fused, confidence), ms_fused = timed(acc.fused)
        acc.close()
        if rep:
            t_add += ta[1:]; t_adds.append(sum(ta)); t_finish.append(ms_finish); t_fused.append(ms_fused)
    w["add"], w["adds_of_a_group"], w["finish"], w["fused"] = stats(t_add), stats(t_adds), stats(t_finish), stats(t_fused)
    w["solve"], w["solve_restrict"] = stats(t_solve[False]), stats(t_solve[True])
    w["solve_over_adds"] = round(w["solve"]["median_ms"] / w["adds_of_a_group"]["median_ms"], 3)
    w["solve_restrict_over_adds"] = round(w["solve_restrict"]["median_ms"] / w["adds_of_a_group"]["median_ms"], 3)
    out["n_labels"] = L
    out["fused_dtype"] = str(fused.dtype)
    out["mean_confidence"] = round(float(confidence.mean()), 4)
    return out


def trace_run(args):
    acc, _ = accumulate(args.images)
    acc.finish()
    print(json.dumps({"solve": acc.solve(tol=0.0, max_iter=args.iterations, restrict=bool(args.restrict))}))
    acc.fused()


def merge(args, out):
    files = glob.glob(os.path.join(args.merge, "**", "*_kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"one *_kernel_trace.csv expected under {args.merge}, found {len(files)}")
    kernels = {}
    for r in csv.DictReader(open(files[0])):
        name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        if "staple_" in name or "labels_collect" in name:
            kernels.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    n, L, V = out["images"], out["n_labels"], out["voxels"]
    A = out["solve_restrict_%d" % args.restrict]["active_voxels"]
    table = {}
    for k, t in sorted(kernels.items()):
        row = {"launches": len(t), "mean_ms": round(float(np.mean(t)), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}
        kind = "estep" if "staple_estep" in k else "mstep" if "staple_mstep" in k else None
        if kind:
            b = moved(kind, n, L, V, A)
            row.update({"bytes_by_count": b, "bytes_per_s": round(b / (row["mean_ms"] * 1e-3), 1),
                        "of_8_TB_per_s": round(b / (row["mean_ms"] * 1e-3) / PEAK_BYTES_PER_S, 4)})
        table[k] = row
    entry = {"restrict": args.restrict, "active_voxels": A, "m_steps": args.iterations, "kernels": table}
    if args.arm:
        out.setdefault("ab", {})[args.arm] = {k: v for k, v in table.items() if "staple_mstep" in k or "staple_estep" in k}
    else:
        out["kernels_under_rocprofv3"] = entry
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "staple.json"))
    ap.add_argument("--images", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--restrict", type=int, default=0)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--merge")
    ap.add_argument("--arm")
    args = ap.parse_args()
    if args.trace_run:
        return trace_run(args)
    out = merge(args, json.load(open(args.out))) if args.merge else measure(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
