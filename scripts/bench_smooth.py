#!/usr/bin/env python3
"""Smoothing the maps before the fit at volume size: scripts/bench_glm.py's case -- the 256^3 grid at 400/256 mm,
20 images, 1 + 7 link chains, the log Jacobian determinant -- with the coverage-aware Gaussian of FWHM 4 mm and 8 mm.

  bench_smooth.py [--out FILE]        wall times (host clock around whole calls; every call ends in a synchronisation):
                                      frog_glm_add_jacobian unsmoothed and smoothed, the median of the 19 later adds;
                                      frog_glm_smooth itself (the scratch); frog_smooth_volume of one map; bin/GroupStats end to
                                      end with 100 permutations, with and without -s
  bench_smooth.py --trace-run         five smoothed adds at each FWHM, nothing else: the command to run under
                                      `rocprofv3 --kernel-trace --stats -d DIR -o p --output-format csv`
  bench_smooth.py --merge-trace DIR   reads DIR's kernel trace (no device needed) and adds the kernel times and the bytes per
                                      second of the smoothing kernels at the bytes the mapping moves
  bench_smooth.py --ab LIB            frog_glm_add_jacobian without smoothing (the median of 9 later adds) and frog_glm_permute
                                      (64 permutations, the median of 9 calls) through the device library LIB (a build of another
                                      commit, which need not export frog_smooth_*): one JSON line
  bench_smooth.py --merge FILE        adds FILE's --ab lines (no device needed) to the output file"""
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

from bench_glm import IMAGES, DISTINCT, design               # noqa: E402
from bench_labels import GRID, N, chain_links, stats, timed  # noqa: E402
import bench_clusters                                        # noqa: E402

FWHMS = (4.0, 8.0)
FWHM = 2.3548200450309493
NEW_SYMBOLS = ("frog_smooth_", "frog_glm_smooth")
KERNELS = ("smooth_x_kernel", "smooth_y_kernel", "smooth_z_kernel", "glm_jacobian_kernel")
ROOFLINE = 8.0e12
# what a pass moves per voxel of a whole-grid range: x reads f32 and writes (num, den); y reads and writes (num, den); z reads
# (num, den) and the f32, writes the f32
PASS_BYTES = {"smooth_x_kernel": 4 + 16, "smooth_y_kernel": 16 + 16, "smooth_z_kernel": 16 + 4 + 4}


def chains_of():
    from frog_amd.chain import Chain, invert
    return [Chain(invert(chain_links(100 + i))) for i in range(DISTINCT)]


def adds(chains, sigma, count=IMAGES):
    """The wall times of the later adds of an accumulator smoothed by sigma (0: unsmoothed), and of frog_glm_smooth."""
    from frog_amd.volume import GroupGLM
    acc = GroupGLM(GRID, design())
    t_smooth = timed(lambda: acc.smooth(sigma))[1] if sigma else 0.0
    t = [timed(lambda: acc.add_jacobian(chains[i % DISTINCT], None, None, True))[1] for i in range(count)][1:]
    plane = acc.plane(count - 1)
    acc.close()
    return t, t_smooth, plane


def measure(args):
    from frog_amd.volume import smooth_taps, smooth_volume
    chains = chains_of()
    out = {"what": "scripts/bench_smooth.py on one MI355X: scripts/bench_glm.py's group (%d images, %d distinct chains of 1 matrix + 7 lattices, "
                   "256^3 grid at 400/256 mm, value = log Jacobian determinant), smoothed at add time; wall times are host-clock times of whole "
                   "calls" % (IMAGES, DISTINCT),
           "voxels": N ** 3, "scratch_bytes": 36 * N ** 3, "bytes_moved_per_smoothed_add": sum(PASS_BYTES.values()) * N ** 3, "wall": {}}
    w = out["wall"]
    t, _, raw = adds(chains, 0.0)
    w["glm_add_jacobian_unsmoothed"] = stats(t)
    for fwhm in FWHMS:
        sigma = fwhm / FWHM
        t, t_smooth, plane = adds(chains, sigma)
        key = "fwhm_%g" % fwhm
        w["glm_add_jacobian_" + key] = dict(stats(t), sigma_mm=round(sigma, 5), radii=[smooth_taps(sigma, s)[0] for s in GRID[2]],
                                            glm_smooth_ms=round(t_smooth, 3))
        w["glm_add_jacobian_" + key]["added_ms"] = round(w["glm_add_jacobian_" + key]["median_ms"] - w["glm_add_jacobian_unsmoothed"]["median_ms"], 3)
        t_volume = [timed(lambda: smooth_volume(raw, sigma, None, GRID[2]))[1] for _ in range(3)][1:]
        again = smooth_volume(raw, sigma, None, GRID[2])
        assert again.tobytes() == plane.tobytes()            # the add's plane is the smoothed raw map, bit for bit
        w["smooth_volume_" + key] = dict(stats(t_volume), note="copies of 67 MB each way included")
        print(key, "done", file=sys.stderr, flush=True)
    if not args.no_tool:
        out["tool"] = {"without_s": bench_clusters.tool(False), "with_s_4": bench_clusters.tool(False, ["-s", "4"]),
                       "with_s_8": bench_clusters.tool(False, ["-s", "8"])}
    return out


def trace_run(args):
    chains = chains_of()
    for fwhm in FWHMS:
        adds(chains, fwhm / FWHM, 5)
    print(json.dumps({"adds_per_fwhm": 5}))


def merge_trace(args, out):
    files = glob.glob(os.path.join(args.merge_trace, "**", "*_kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"one *_kernel_trace.csv expected under {args.merge_trace}, found {len(files)}")
    kernels = {}
    for r in sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"])):
        name = next((k for k in KERNELS if k in r["Kernel_Name"]), None)
        if name:
            kernels.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    table = {}
    for name, t in sorted(kernels.items()):
        # trace_run's launches: five adds at the first FWHM, then five at the second
        half = len(t) // 2
        for fwhm, part in zip(FWHMS, (t[:half], t[half:])):
            e = {"launches": len(part), "median_ms": round(float(np.median(part)), 4), "min_ms": round(min(part), 4), "max_ms": round(max(part), 4)}
            if name in PASS_BYTES:
                e["bytes"] = PASS_BYTES[name] * N ** 3
                e["bytes_per_s"] = round(e["bytes"] / (e["median_ms"] * 1e-3), 1)
                e["share_of_8_TB_per_s"] = round(e["bytes_per_s"] / ROOFLINE, 4)
            table.setdefault("fwhm_%g" % fwhm, {})[name] = e
    for e in table.values():
        passes = [e[k] for k in PASS_BYTES if k in e]
        e["smoothing_ms"] = round(sum(p["median_ms"] for p in passes), 4)
        e["smoothing_at_the_roofline_ms"] = round(sum(p["bytes"] for p in passes) / ROOFLINE * 1e3, 4)
    out["kernels_under_rocprofv3"] = table


def ab(args):
    """The unsmoothed add and frog_glm_permute, which existed before frog_smooth, through another build of the device library."""
    os.environ["FROG_HIP_LIB"] = os.path.abspath(args.ab)
    from frog_amd import _abi
    _abi.HIP_SYMBOLS = {k: v for k, v in _abi.HIP_SYMBOLS.items() if not k.startswith(NEW_SYMBOLS)}
    from bench_glm import filled
    from frog_amd.volume import glm_draw
    t_add = []
    acc = filled(chains_of(), t_add)
    perm, _ = glm_draw(IMAGES, 64, 1)
    t = [timed(lambda: acc.permute([[0.0, 1.0, 0.0]], perm, None, [1]))[1] for _ in range(10)][1:]
    acc.close()
    print(json.dumps({"library": args.ab, "glm_add_jacobian": stats(t_add[-9:]), "glm_permute_64": stats(t)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_smooth.json"))
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
            out["add_and_permute_by_library_in_turn"] = [json.loads(line) for line in open(args.merge) if line.strip().startswith("{")]
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
