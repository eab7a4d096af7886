#!/usr/bin/env python3
"""frog_rank at volume size: the 256^3 grid and the 1 + 7 link chain of scripts/bench_labels.py, int16 images of
256^3 voxels (scripts/bench_cover.py's), trilinear, at 20, 100 and 500 images; the 100-image case also in 4 slabs.

  bench_rank.py [--out FILE]          wall times (host clock around whole calls; every call ends in a synchronisation):
                                      frog_rank_add next to frog_cover_add on the same volume and chain, in turn;
                                      frog_rank_finish (median and MAD), the median of 7 calls; a device-to-device hipMemcpy
                                      of the bytes the finish kernel moves (capped at 8 GiB), the median of 7
  bench_rank.py --trace-run           one accumulation and one finish per case, nothing else: the command to run under
                                      `rocprofv3 --kernel-trace --stats -d DIR -o p --output-format csv`
  bench_rank.py --merge DIR           reads DIR's kernel trace (no device needed) and adds the kernel times and the rates"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_cover import image_volume                                # noqa: E402
from bench_labels import GRID, N, chain_links, stats, timed         # noqa: E402

CASES = (20, 100, 500)
DISTINCT = 4                        # volumes and chains, taken in turn: the collect's work does not depend on the values
COPY_CAP = 8 << 30


def moved_bytes(n):
    """What a finish kernel with the median and the MAD moves: 4 bytes per image and voxel read, f32 + f32 + u16 written."""
    return N ** 3 * (4 * n + 10)


def inputs():
    from frog_amd.chain import Chain, invert
    o, s = GRID[1], GRID[2]
    return [(image_volume(i), o, s) for i in range(DISTINCT)], [Chain(invert(chain_links(100 + i))) for i in range(DISTINCT)]


def filled(n, vols, chains, window=None, times=None):
    from frog_amd.volume import RankImages
    acc = RankImages(GRID, n, window)
    for i in range(n):
        ms = timed(lambda: acc.add(vols[i % DISTINCT], chains[i % DISTINCT], None, 1, 0.0))[1]
        if times is not None and i:                         # the first add allocates the staging
            times.append(ms)
    return acc


def copy_yardstick(n_bytes, repeats):
    hip = C.CDLL("libamdhip64.so")
    a, b = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(a), C.c_size_t(n_bytes)) == 0 and hip.hipMalloc(C.byref(b), C.c_size_t(n_bytes)) == 0
    hip.hipMemset(a, 1, C.c_size_t(n_bytes)); hip.hipMemset(b, 2, C.c_size_t(n_bytes)); hip.hipDeviceSynchronize()

    def once():
        assert hip.hipMemcpy(b, a, C.c_size_t(n_bytes), 3) == 0     # hipMemcpyDeviceToDevice
        hip.hipDeviceSynchronize()
    once()
    t = [timed(once)[1] for _ in range(repeats)]
    hip.hipFree(a); hip.hipFree(b)
    return t


def measure(args):
    from frog_amd.volume import CoverAverage
    vols, chains = inputs()
    out = {"what": "scripts/bench_rank.py on one MI355X: int16 images of 256^3 voxels (%d distinct, in turn), each through the inverse of 1 "
                   "matrix + 7 lattices onto a 256^3 grid at 400/256 mm, trilinear; wall times are host-clock times of whole calls, "
                   "copies included; finish = median + MAD + count" % DISTINCT,
           "voxels": N ** 3, "register_tier_up_to": 64, "wall": {}, "cases": {}}
    cov, t_cover, t_rank = CoverAverage(GRID), [], []
    for i in range(13):
        ms = timed(lambda: cov.add(vols[i % DISTINCT], chains[i % DISTINCT], None, 1, 0.0))[1]
        if i:
            t_cover.append(ms)
    cov.close()
    for n in CASES:
        acc = filled(n, vols, chains, None, t_rank if n == CASES[0] else None)
        t = [timed(lambda: acc.finish(1, 0.0, (0.5,)))[1] for _ in range(args.repeats + 1)][1:]
        acc.close()
        b = moved_bytes(n)
        tc = copy_yardstick(min(b, COPY_CAP), args.repeats)
        out["cases"][str(n)] = {"finish_wall": stats(t), "bytes_moved": b, "copy_bytes": min(b, COPY_CAP), "copy_wall": stats(tc),
                                "copy_bytes_per_s": round(min(b, COPY_CAP) / (float(np.median(tc)) * 1e-3), 1)}
    t = []
    for rep in range(3):                                    # 100 images in 4 slabs of 64 planes: adds and finishes, whole
        def slabs():
            for first in range(0, N, N // 4):
                acc = filled(100, vols, chains, (first, N // 4))
                acc.finish(1, 0.0, (0.5,))
                acc.close()
        t.append(timed(slabs)[1])
    out["cases"]["100_in_4_slabs"] = {"adds_and_finishes_wall": stats(t)}
    w = out["wall"]
    w["cover_add"], w["rank_add"] = stats(t_cover), stats(t_rank)
    w["rank_add_over_cover_add"] = round(w["rank_add"]["median_ms"] / w["cover_add"]["median_ms"], 3)
    return out


def trace_run(args):
    from frog_amd.volume import CoverAverage
    vols, chains = inputs()
    cov = CoverAverage(GRID)
    for i in range(4):
        cov.add(vols[i], chains[i], None, 1, 0.0)
    cov.close()
    for n in CASES:
        acc = filled(n, vols, chains)
        acc.finish(1, 0.0, (0.5,))
        acc.close()
    acc = filled(100, vols, chains, (0, N // 4))
    acc.finish(1, 0.0, (0.5,))
    acc.close()


def merge(directory, out):
    files = glob.glob(os.path.join(directory, "**", "*_kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"one *_kernel_trace.csv expected under {directory}, found {len(files)}")
    kernels, finishes = {}, []
    for r in sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"])):
        name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        if "rank_finish" in name:
            finishes.append((name, ms))
        elif "rank_reslice" in name or "cover_reslice" in name:
            kernels.setdefault(name, []).append(ms)
    out["kernels_under_rocprofv3"] = {k: {"launches": len(t), "median_ms": round(float(np.median(t)), 4), "min_ms": round(min(t), 4),
                                          "max_ms": round(max(t), 4)} for k, t in sorted(kernels.items())}
    # one finish launch per case, in the order of trace_run: 20, 100, 500 whole, then one quarter of 100
    for (name, ms), (key, n, share) in zip(finishes, [(str(c), c, 1.0) for c in CASES] + [("100_in_4_slabs", 100, 0.25)]):
        b = moved_bytes(n) * share
        case = out["cases"].setdefault(key, {})
        case.update({"finish_kernel": name, "finish_kernel_ms": round(ms, 4), "finish_kernel_bytes": int(b),
                     "finish_kernel_bytes_per_s": round(b / (ms * 1e-3), 1)})
        if "copy_bytes_per_s" in case:
            case["finish_over_copy_rate"] = round(b / (ms * 1e-3) / case["copy_bytes_per_s"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank.json"))
    ap.add_argument("--repeats", type=int, default=7)
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
