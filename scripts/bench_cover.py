#!/usr/bin/env python3
"""frog_cover at volume size, by section 15's protocol: the 256^3 grid and the 1 + 7 link chain of
scripts/bench_labels.py (one seeded chain per image, inverted), int16 images of 256^3 voxels, trilinear.

  bench_cover.py [--out FILE]         wall times (host clock around whole calls; every call ends in a synchronisation):
                                      frog_cover_add, frog_cover_add with a mask and frog_average_add on the same volume and
                                      chain, in one process, in turn; the median of the calls, the ratios to
                                      frog_average_add, and that call's own spread between the rounds; frog_cover_finish
  bench_cover.py --trace-run          one accumulation of each kind, nothing else: the command to run under
                                      `rocprofv3 --kernel-trace --stats -d DIR -o p --output-format csv`
  bench_cover.py --merge DIR          reads DIR's kernel trace (no device needed) and adds the kernel times"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_labels import GRID, N, chain_links, stats, timed          # noqa: E402

MASK_N = 160
MASK_GEOMETRY = ((20.0, 30.0, 10.0), (2.25, 2.0, 2.4))          # origin, spacing: not the source's


def image_volume(image):
    z, y, x = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij", sparse=True)
    return (1000 + 600 * np.sin((x + 5 * image) / 7.0) * np.cos(y / 9.0) + 3 * z + 40 * image).astype(np.int16)


def mask_volume(image):
    """A ball of non-zero voxels (two thirds of the mask's width), off centre per image."""
    z, y, x = np.meshgrid(np.arange(MASK_N), np.arange(MASK_N), np.arange(MASK_N), indexing="ij", sparse=True)
    c = MASK_N / 2 + image
    return (((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2) < (MASK_N / 3) ** 2).astype(np.uint8)


def measure(args):
    from frog_amd.chain import Chain, invert
    from frog_amd.volume import Average, CoverAverage
    n = args.images
    o, s = GRID[1], GRID[2]
    vols = [(image_volume(i), o, s) for i in range(n)]
    masks = [(mask_volume(i),) + MASK_GEOMETRY for i in range(n)]
    chains = [Chain(invert(chain_links(100 + i))) for i in range(n)]
    out = {"what": "scripts/bench_cover.py on one MI355X: %d int16 images of 256^3 voxels, each through the inverse of 1 matrix + 7 "
                   "lattices (4, 4, 8, 8, 16, 16, 16 cells over 400 mm) onto a 256^3 grid at 400/256 mm, trilinear; masks uint8 %d^3 "
                   "of another geometry; wall times are host-clock times of whole calls, copies included" % (n, MASK_N),
           "images": n, "voxels": N ** 3, "wall": {}}
    w = out["wall"]
    t_cover, t_masked, t_average, t_finish, round_medians = [], [], [], [], []
    for rep in range(args.repeats + 1):                     # the first round warms up (code objects, first allocations)
        cov, msk, avg = CoverAverage(GRID), CoverAverage(GRID), Average(GRID, n)
        tc, tm, ta = [], [], []
        for v, m, c in zip(vols, masks, chains):
            tc.append(timed(lambda: cov.add(v, c, None, 1, 0.0))[1])
            tm.append(timed(lambda: msk.add(v, c, m, 1, 0.0))[1])
            ta.append(timed(lambda: avg.add(v, c, 1, 0.0))[1])
        (mean, stdev, count), ms_finish = timed(cov.finish)
        masked_count = msk.finish()[2]
        avg.finish()
        cov.close(); msk.close(); avg.close()
        if rep:
            t_cover += tc[1:]; t_masked += tm[1:]; t_average += ta[1:]      # the first add of an accumulator allocates its staging
            t_finish.append(ms_finish)
            round_medians.append(round(float(np.median(ta[1:])), 3))
    w["cover_add"], w["cover_add_masked"], w["average_add"] = stats(t_cover), stats(t_masked), stats(t_average)
    w["average_add_round_medians_ms"] = round_medians
    w["average_add_spread"] = round((max(round_medians) - min(round_medians)) / w["average_add"]["median_ms"], 4)
    w["cover_add_over_average_add"] = round(w["cover_add"]["median_ms"] / w["average_add"]["median_ms"], 3)
    w["cover_add_masked_over_average_add"] = round(w["cover_add_masked"]["median_ms"] / w["average_add"]["median_ms"], 3)
    w["finish"] = stats(t_finish)
    out["mean_count"] = round(float(count.mean()), 3)
    out["mean_count_masked"] = round(float(masked_count.mean()), 3)
    out["nan_in_stdev"] = int(np.isnan(stdev).sum())
    return out


def trace_run(args):
    from frog_amd.chain import Chain, invert
    from frog_amd.volume import Average, CoverAverage
    n = args.images
    cov, msk, avg = CoverAverage(GRID), CoverAverage(GRID), Average(GRID, n)
    for i in range(n):
        v, c = (image_volume(i), GRID[1], GRID[2]), Chain(invert(chain_links(100 + i)))
        cov.add(v, c, None, 1, 0.0)
        msk.add(v, c, (mask_volume(i),) + MASK_GEOMETRY, 1, 0.0)
        avg.add(v, c, 1, 0.0)
        c.close()
    cov.finish()
    msk.finish()
    avg.finish()


def merge(directory, out):
    files = glob.glob(os.path.join(directory, "**", "*_kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"one *_kernel_trace.csv expected under {directory}, found {len(files)}")
    kernels = {}
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    n_cover = 0
    for r in rows:
        name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        if "cover_reslice" in name:                         # launched in turn: without a mask, then with one
            name += " (masked)" if n_cover % 2 else " (no mask)"
            n_cover += 1
        if "cover_" in name or "reslice_accumulate" in name or "average_finish" in name:
            kernels.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    out["kernels_under_rocprofv3"] = {k: {"launches": len(t), "mean_ms": round(float(np.mean(t)), 4), "median_ms": round(float(np.median(t)), 4),
                                          "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)} for k, t in sorted(kernels.items())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cover_average.json"))
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
