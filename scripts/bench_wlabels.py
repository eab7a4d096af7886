#!/usr/bin/env python3
"""frog_wlabels at volume size: the inputs of scripts/bench_labels.py -- a 256^3 grid, one seeded chain of
1 matrix + 7 lattices per atlas, inverted -- with 20 atlases of an int16 image and a uint16 label map, radius 2.

  bench_wlabels.py [--out FILE]       wall times (host clock around whole calls; every call ends in a synchronisation or a
                                      device-to-host copy): per frog_wlabels_add, beside frog_average_add + frog_labels_add on
                                      the same atlas and chain in the same process and in turn; target, finish, fused,
                                      probability
  bench_wlabels.py --trace-run        the target and three adds at each of radius 1, 2 and 4, and every getter once: the
                                      command to run under `rocprofv3 --kernel-trace` or under `rocprofv3 --pmc ...`
  bench_wlabels.py --merge DIR        reads DIR's kernel trace, counter files and ab.jsonl (no device needed), adds them to --out
  bench_wlabels.py --ab LIB           frog_labels_add and frog_chain_reslice through the device library LIB (a path), loaded
                                      with ctypes alone so that a library from before frog_wlabels loads too; prints one
                                      JSON line.  Run it once per library, in turn, to set two builds side by side."""
import argparse
import collections
import csv
import ctypes as C
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_labels import GRID, N, chain_links, label_volume, stats, timed      # noqa: E402


def image_volume(k):
    """An int16 image that follows the label blocks of atlas k, with noise: neighbouring atlases correlate locally."""
    rng = np.random.default_rng(500 + k)
    return (label_volume(k).astype(np.int32) % 997 + rng.integers(0, 200, (N, N, N), dtype=np.int32)).astype(np.int16)


def measure(args):
    from frog_amd.chain import Chain, invert
    from frog_amd.volume import Average, Labels, WeightedLabels
    n = args.images
    o, s = GRID[1], GRID[2]
    maps = [(label_volume(i), o, s) for i in range(n)]
    images = [(image_volume(i), o, s) for i in range(n)]
    target = (image_volume(n), o, s)
    chains = [Chain(invert(chain_links(100 + i))) for i in range(n)]
    target_chain = Chain(invert(chain_links(99)))
    out = {"what": "scripts/bench_wlabels.py on one MI355X: %d atlases (int16 image + uint16 label map of 256^3 voxels), each through the "
                   "inverse of 1 matrix + 7 lattices (4, 4, 8, 8, 16, 16, 16 cells over 400 mm) onto a 256^3 grid at 400/256 mm, radius %d, "
                   "power 2; wall times are host-clock times of whole calls, copies included" % (n, args.radius),
           "images": n, "voxels": N ** 3, "radius": args.radius, "wall": {}}
    w = out["wall"]
    t_w, t_avg, t_lab, t_target, t_finish, t_fused, t_prob = [], [], [], [], [], [], []
    for rep in range(args.repeats + 1):                     # the first round warms up (code objects, first allocations)
        acc, avg, lab = WeightedLabels(GRID, n, 0, args.radius, 2), Average(GRID, n), Labels(GRID, n)
        _, ms_target = timed(lambda: acc.target(target, target_chain, 1, 0.0))
        tw, ta, tl = [], [], []
        for k in range(n):
            tw.append(timed(lambda: acc.add(images[k], maps[k], chains[k], 1, 0.0, 0.0))[1])
            ta.append(timed(lambda: avg.add(images[k], chains[k], 1, 0.0))[1])
            tl.append(timed(lambda: lab.add(maps[k], chains[k], 0.0))[1])
        n_labels, ms_finish = timed(acc.finish)
        (fused, confidence), ms_fused = timed(acc.fused)
        _, ms_prob = timed(lambda: acc.probability(int(acc.values()[0])))
        avg.finish(); lab.finish()
        acc.close(); avg.close(); lab.close()
        if rep:
            t_w += tw[1:]; t_avg += ta[1:]; t_lab += tl[1:]  # the first add of an accumulator allocates the label planes
            t_target.append(ms_target); t_finish.append(ms_finish); t_fused.append(ms_fused); t_prob.append(ms_prob)
    w["wlabels_add"], w["average_add"], w["labels_add"] = stats(t_w), stats(t_avg), stats(t_lab)
    w["average_add_plus_labels_add_ms"] = round(w["average_add"]["median_ms"] + w["labels_add"]["median_ms"], 3)
    w["wlabels_add_over_the_two"] = round(w["wlabels_add"]["median_ms"] / w["average_add_plus_labels_add_ms"], 3)
    w["target"], w["finish"], w["fused"], w["probability"] = stats(t_target), stats(t_finish), stats(t_fused), stats(t_prob)
    out["n_labels"] = n_labels
    out["fused_dtype"] = str(fused.dtype)
    out["mean_confidence"] = round(float(confidence.mean()), 4)
    return out


def trace_run(args):
    from frog_amd.chain import Chain, invert
    from frog_amd.volume import WeightedLabels
    o, s = GRID[1], GRID[2]
    target = (image_volume(3), o, s)
    atlases = [((image_volume(i), o, s), (label_volume(i), o, s), Chain(invert(chain_links(100 + i)))) for i in range(3)]
    target_chain = Chain(invert(chain_links(99)))
    for radius in (1, 2, 4):
        acc = WeightedLabels(GRID, 3, 0, radius, 2)
        acc.target(target, target_chain, 1, 0.0)
        for image, labels, chain in atlases:
            acc.add(image, labels, chain, 1, 0.0, 0.0)
        acc.finish()
        acc.fused()
        acc.probability(0)
        acc.close()


def short(name):
    return name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]


def merge(directory, out):
    kernels = {}
    for f in glob.glob(os.path.join(directory, "**", "*_kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "wlabels_" in r["Kernel_Name"]:
                kernels.setdefault(short(r["Kernel_Name"]), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    if kernels:
        out["kernels_under_rocprofv3"] = {k: {"launches": len(t), "mean_ms": round(float(np.mean(t)), 4), "min_ms": round(min(t), 4),
                                              "max_ms": round(max(t), 4)} for k, t in sorted(kernels.items())}
    counters = collections.defaultdict(lambda: collections.defaultdict(lambda: [0.0, 0]))
    for f in glob.glob(os.path.join(directory, "**", "*_counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "wlabels_vote" in r["Kernel_Name"]:
                c = counters[short(r["Kernel_Name"])][r["Counter_Name"]]
                c[0] += float(r["Counter_Value"]); c[1] += 1
    if counters:
        out["vote_kernel_counters_per_launch"] = {k: {name: round(v / m, 1) for name, (v, m) in sorted(c.items())} for k, c in sorted(counters.items())}
    ab_lines = os.path.join(directory, "ab.jsonl")             # profile_wlabels.sh's second argument: --ab runs in turn
    if os.path.exists(ab_lines):
        out["labels_add_and_reslice_by_library_in_turn"] = [json.loads(line) for line in open(ab_lines) if line.strip()]
    return out


def ab(args):
    """frog_labels_add and frog_chain_reslice through args.ab, by ctypes alone."""
    from frog_amd import _abi
    lib = C.CDLL(os.path.abspath(args.ab))
    for name in ("frog_chain_create", "frog_chain_destroy", "frog_chain_invert_links", "frog_chain_reslice", "frog_labels_create", "frog_labels_add",
                 "frog_labels_destroy"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _abi.HIP_SYMBOLS[name]
    links = chain_links(100)
    src = (_abi.FrogChainLink * len(links))(*[l.view() for l in links])
    dst = (_abi.FrogChainLink * len(links))()
    assert lib.frog_chain_invert_links(src, len(links), dst) == 0
    chain = C.c_void_p()
    assert lib.frog_chain_create(dst, len(links), 0, C.byref(chain)) == 0
    labels = np.ascontiguousarray(label_volume(0))
    image = image_volume(0)
    out_image = np.empty_like(image)
    grid = _abi.volume_view(None, GRID[1], GRID[2], GRID[0])
    lv, iv, ov = (_abi.volume_view(a, GRID[1], GRID[2]) for a in (labels, image, out_image))
    t_add, t_reslice = [], []
    for rep in range(args.repeats + 1):
        acc = C.c_void_p()
        assert lib.frog_labels_create(C.byref(grid), 8, 0, 0, C.byref(acc)) == 0
        for k in range(8):
            rc, ms = timed(lambda: lib.frog_labels_add(acc, chain, C.byref(lv), 0.0, None))
            assert rc == 0
            if rep and k:
                t_add.append(ms)
            rc, ms = timed(lambda: lib.frog_chain_reslice(chain, C.byref(iv), C.byref(ov), 1, 0.0))
            assert rc == 0
            if rep:
                t_reslice.append(ms)
        lib.frog_labels_destroy(acc)
    lib.frog_chain_destroy(chain)
    print(json.dumps({"library": args.ab, "labels_add": stats(t_add), "chain_reslice": stats(t_reslice)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weighted_fusion.json"))
    ap.add_argument("--images", type=int, default=20)
    ap.add_argument("--radius", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--merge")
    ap.add_argument("--ab")
    args = ap.parse_args()
    if args.trace_run:
        return trace_run(args)
    if args.ab:
        return ab(args)
    out = merge(args.merge, json.load(open(args.out))) if args.merge else measure(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
