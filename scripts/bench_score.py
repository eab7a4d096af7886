#!/usr/bin/env python3
"""frog_cover_score at volume size, by scripts/bench_cover.py's protocol and inputs: the 256^3 grid, 12 int16
images, the inverted 1 + 7 link chains, the 160^3 masks, trilinear; the calls in turn in one process.

  bench_score.py [--out FILE]         wall times (host clock around whole calls; every call ends in a synchronisation or a
                                      copy back): frog_cover_add (the yardstick) and frog_cover_score on the same volume and
                                      chain, without and with the mask, and frog_cover_score without a chain (the volume on
                                      the grid: the reduction and the histogram are the whole kernel); medians, the ratios to
                                      frog_cover_add and that call's own spread between the rounds
  bench_score.py --trace-run          one pass of each kind, nothing else: the command to run under
                                      `rocprofv3 --kernel-trace --stats -d DIR -o p --output-format csv`
  bench_score.py --merge DIR          reads DIR's kernel trace (no device needed) and adds the kernel times"""
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

from bench_labels import GRID, N, chain_links, stats, timed          # noqa: E402
from bench_cover import MASK_GEOMETRY, MASK_N, image_volume, mask_volume      # noqa: E402

BINS, RANGE = 64, (0.0, 2500.0)
CHAINLESS_BYTES = N ** 3 * (2 + 4 + 2)          # per voxel: the int16 source, the f32 mean, the u16 count
STREAM_TBS = 8.0                                # the streaming figure DESIGN.md 6 divides by


def measure(args):
    from frog_amd.chain import Chain, invert
    from frog_amd.volume import CoverAverage
    n = args.images
    o, s = GRID[1], GRID[2]
    vols = [(image_volume(i), o, s) for i in range(n)]
    masks = [(mask_volume(i),) + MASK_GEOMETRY for i in range(n)]
    chains = [Chain(invert(chain_links(100 + i))) for i in range(n)]
    out = {"what": "scripts/bench_score.py on one MI355X: %d int16 images of 256^3 voxels, each through the inverse of 1 matrix + 7 "
                   "lattices onto a 256^3 grid, trilinear; masks uint8 %d^3 of another geometry; frog_cover_score with leave_one_out, "
                   "%d x %d bins over [%g, %g); wall times are host-clock times of whole calls, copies included"
                   % (n, MASK_N, BINS, BINS, RANGE[0], RANGE[1]),
           "images": n, "voxels": N ** 3, "tile_voxels": 2048, "wall": {}}
    w = out["wall"]
    t = {k: [] for k in ("cover_add", "cover_add_masked", "score", "score_masked", "score_no_histogram", "score_chainless")}
    round_medians = []
    scores = None
    for rep in range(args.repeats + 1):                     # the first round warms up (code objects, first allocations)
        cov, msk = CoverAverage(GRID), CoverAverage(GRID)
        r = {k: [] for k in t}
        for v, m, c in zip(vols, masks, chains):
            r["cover_add"].append(timed(lambda: cov.add(v, c, None, 1, 0.0))[1])
            r["cover_add_masked"].append(timed(lambda: msk.add(v, c, m, 1, 0.0))[1])
        scores = []
        for v, m, c in zip(vols, masks, chains):
            # the metrics (host, microseconds) are part of Python's score(): the device call dominates
            row, ms = timed(lambda: cov.score(v, c, None, 1, 0.0, 1, True, BINS, RANGE))
            r["score"].append(ms)
            scores.append(row)
            r["score_masked"].append(timed(lambda: msk.score(v, c, m, 1, 0.0, 1, True, BINS, RANGE))[1])
            r["score_no_histogram"].append(timed(lambda: cov.score(v, c, None, 1, 0.0, 1, True, 0))[1])
            r["score_chainless"].append(timed(lambda: cov.score(v[0], None, None, 1, 0.0, 1, False, BINS, RANGE))[1])
        cov.close(); msk.close()
        if rep:
            for k in t:
                t[k] += r[k][1:]                            # the first call of an accumulator allocates its staging
            round_medians.append(round(float(np.median(r["cover_add"][1:])), 3))
    for k in t:
        w[k] = stats(t[k])
    w["cover_add_round_medians_ms"] = round_medians
    w["cover_add_spread"] = round((max(round_medians) - min(round_medians)) / w["cover_add"]["median_ms"], 4)
    w["score_over_cover_add"] = round(w["score"]["median_ms"] / w["cover_add"]["median_ms"], 3)
    w["score_masked_over_cover_add_masked"] = round(w["score_masked"]["median_ms"] / w["cover_add_masked"]["median_ms"], 3)
    w["score_no_histogram_over_cover_add"] = round(w["score_no_histogram"]["median_ms"] / w["cover_add"]["median_ms"], 3)
    out["ncc"] = [round(row["ncc"], 6) for row in scores]
    out["nmi"] = [round(row["nmi"], 6) for row in scores]
    out["covered_fraction"] = [round(row["covered_fraction"], 4) for row in scores]
    return out


def trace_run(args):
    from frog_amd.chain import Chain, invert
    from frog_amd.volume import CoverAverage
    n = args.images
    cov, msk = CoverAverage(GRID), CoverAverage(GRID)
    items = []
    for i in range(n):
        v, c = (image_volume(i), GRID[1], GRID[2]), Chain(invert(chain_links(100 + i)))
        m = (mask_volume(i),) + MASK_GEOMETRY
        cov.add(v, c, None, 1, 0.0)
        msk.add(v, c, m, 1, 0.0)
        items.append((v, c, m))
    for v, c, m in items:                                   # in turn: no mask, masked, no histogram, chainless
        cov.score(v, c, None, 1, 0.0, 1, True, BINS, RANGE)
        msk.score(v, c, m, 1, 0.0, 1, True, BINS, RANGE)
        cov.score(v, c, None, 1, 0.0, 1, True, 0)
        cov.score(v[0], None, None, 1, 0.0, 1, False, BINS, RANGE)


def merge(directory, out):
    files = glob.glob(os.path.join(directory, "**", "*_kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"one *_kernel_trace.csv expected under {directory}, found {len(files)}")
    kernels = {}
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    n_add = n_score = 0
    for r in rows:
        name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        if "cover_reslice" in name:                         # launched in turn: without a mask, then with one
            name += (" (no mask)", " (masked)")[n_add % 2]
            n_add += 1
        elif "cover_score_kernel" in name:
            name += (" (no mask)", " (masked)", " (no histogram)")[n_score % 3]
            n_score += 1
        if "cover_" in name:
            kernels.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    k = out["kernels_under_rocprofv3"] = {name: {"launches": len(t), "mean_ms": round(float(np.mean(t)), 4), "median_ms": round(float(np.median(t)), 4),
                                                 "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)} for name, t in sorted(kernels.items())}
    find = lambda part: next((v["median_ms"] for name, v in k.items() if part in name), None)
    add, score, chainless = find("cover_reslice_kernel<short> (no mask)"), find("cover_score_kernel<short> (no mask)"), find("cover_score_identity")
    if add and score:
        out["score_kernel_over_add_kernel"] = round(score / add, 3)
    if chainless:
        out["chainless_tb_per_s"] = round(CHAINLESS_BYTES / (chainless * 1e-3) / 1e12, 3)
        out["chainless_share_of_%g_tb_per_s" % STREAM_TBS] = round(out["chainless_tb_per_s"] / STREAM_TBS, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_quality.json"))
    ap.add_argument("--images", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--merge")
    args = ap.parse_args()
    if args.trace_run:
        return trace_run(args)
    out = merge(args.merge, json.load(open(args.out))) if args.merge else measure(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
