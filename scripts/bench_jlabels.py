#!/usr/bin/env python3
"""frog_jlabels at volume size: the inputs of scripts/bench_wlabels.py -- a 256^3 grid, one seeded chain of
1 matrix + 7 lattices per atlas, inverted, 20 atlases of an int16 image and a uint16 label map -- radius 2, beta 2, alpha 0.1.

  bench_jlabels.py [--out FILE] [--depth NZ]  wall times (host clock around whole calls): target, per frog_jlabels_add, finish
                                      (the joint solve), fused, probability, weight.  --depth cuts the grid to NZ planes (the
                                      sources stay 256^3): the solve's time is proportional, so a shallow grid prices a deep one
  bench_jlabels.py --trace-run [--depth NZ]   one accumulation and the getters once: the command to run under `rocprofv3
                                      --kernel-trace` or, in a run of its own, under `rocprofv3 --pmc ...`
  bench_jlabels.py --tool [--depth NZ]        bin/AtlasSegment on the same inputs as files, with -j 1 and without: wall times
                                      and phase lines; prints one JSON line
  bench_jlabels.py --merge DIR        reads DIR's kernel trace, counter files, tool.json and ab.jsonl (no device needed), adds
                                      them to --out
  bench_jlabels.py --ab LIB           frog_labels_add, frog_wlabels_add and frog_chain_reslice through the device library LIB (a
                                      path), loaded with ctypes alone so that a library from before frog_jlabels loads too;
                                      prints one JSON line.  Run it once per library, in turn."""
import argparse
import collections
import csv
import ctypes as C
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_labels import GRID, N, chain_links, label_volume, stats, timed      # noqa: E402
from bench_wlabels import image_volume, short                                   # noqa: E402

# separately rounded f64 operations per second of the vector ALU: 256 CUs x 4 SIMDs x 64 lanes / 4 cycles x 2.4 GHz (an
# addition or a product of a wavefront issues in 4 cycles; half the FMA figure, since nothing here contracts)
F64_OPS_PER_S = 256 * 4 * 16 * 2.4e9


def grid_of(depth):
    return ((N, N, depth), GRID[1], GRID[2])


def gram_operations(dims, n, radius):
    """The products and additions of the Gram pass: 2 per pair and patch voxel inside the grid."""
    taps = 1
    for length in dims:
        taps *= sum(min(i + radius, length - 1) - max(i - radius, 0) + 1 for i in range(length))
    return 2 * taps * n * (n + 1) // 2


def inputs(n):
    from frog_amd.chain import Chain, invert
    o, s = GRID[1], GRID[2]
    maps = [(label_volume(i), o, s) for i in range(n)]
    images = [(image_volume(i), o, s) for i in range(n)]
    chains = [Chain(invert(chain_links(100 + i))) for i in range(n)]
    return (image_volume(n), o, s), Chain(invert(chain_links(99))), images, maps, chains


def measure(args):
    from frog_amd.volume import JointLabels
    n, grid = args.images, grid_of(args.depth)
    target, target_chain, images, maps, chains = inputs(n)
    out = {"what": "scripts/bench_jlabels.py on one MI355X: %d atlases (int16 image + uint16 label map of 256^3 voxels), each through the "
                   "inverse of 1 matrix + 7 lattices (4, 4, 8, 8, 16, 16, 16 cells over 400 mm) onto a 256 x 256 x %d grid at 400/256 mm, "
                   "radius %d, beta 2, alpha 0.1; wall times are host-clock times of whole calls, copies included"
                   % (n, args.depth, args.radius),
           "images": n, "grid": list(grid[0]), "radius": args.radius, "wall": {}}
    t_add, t_target, t_finish, t_fused, t_prob, t_weight = [], [], [], [], [], []
    for rep in range(args.repeats):
        acc = JointLabels(grid, n, 0, args.radius, 2, 0.1, True)
        t_target.append(timed(lambda: acc.target(target, target_chain, 1, 0.0))[1])
        ta = [timed(lambda: acc.add(images[k], maps[k], chains[k], 1, 0.0, 0.0))[1] for k in range(n)]
        t_add += ta[1:]                                      # the first add of an accumulator allocates the label planes
        n_labels, ms = timed(acc.finish)
        t_finish.append(ms)
        (fused, confidence), ms = timed(acc.fused)
        t_fused.append(ms)
        t_prob.append(timed(lambda: acc.probability(int(acc.values()[0])))[1])
        w0, ms = timed(lambda: acc.weight(0))
        t_weight.append(ms)
        acc.close()
    w = out["wall"]
    w["target"], w["jlabels_add"], w["finish"] = stats(t_target), stats(t_add), stats(t_finish)
    w["fused"], w["probability"], w["weight"] = stats(t_fused), stats(t_prob), stats(t_weight)
    ops = gram_operations(grid[0], n, args.radius)
    out["gram_f64_operations"] = ops
    out["finish_gram_operations_per_s"] = round(ops / (w["finish"]["min_ms"] * 1e-3), 1)
    out["n_labels"] = n_labels
    out["mean_confidence"] = round(float(confidence.mean()), 4)
    out["negative_weights_share_of_atlas_0"] = round(float((w0 < 0).mean()), 4)
    return out


def trace_run(args):
    from frog_amd.volume import JointLabels
    n, grid = args.images, grid_of(args.depth)
    target, target_chain, images, maps, chains = inputs(n)
    acc = JointLabels(grid, n, 0, args.radius, 2, 0.1, True)
    acc.target(target, target_chain, 1, 0.0)
    for k in range(n):
        acc.add(images[k], maps[k], chains[k], 1, 0.0, 0.0)
    acc.finish()
    acc.fused()
    acc.probability(0)
    acc.close()


def tool(args):
    """bin/AtlasSegment on the same atlases and chains as files, with -j 1 and without."""
    from frog_amd.volume import write_volume
    n = args.images
    d = tempfile.mkdtemp(prefix="bench_jlabels_")
    try:
        os.makedirs(os.path.join(d, "transforms"))
        names = []
        o, s = GRID[1], GRID[2]
        write_volume(os.path.join(d, "target.nii.gz"), image_volume(n), o, s)
        for i in range(n):
            names.append(f"v{i}.nii.gz")
            write_volume(os.path.join(d, names[-1]), image_volume(i), o, s)
            write_volume(os.path.join(d, f"l{i}.nii.gz"), label_volume(i), o, s)
            ts = []
            for l in chain_links(100 + i):
                if l.matrix is not None:
                    ts.append({"type": "vtkMatrixToLinearTransform", "matrix": l.matrix.ravel().tolist()})
                else:
                    ts.append({"type": "vtkBSplineTransform", "dimensions": list(l.dims), "origin": list(l.origin), "spacing": list(l.spacing),
                               "coeffs": [float(c) for c in l.coeffs.ravel()]})
            with open(os.path.join(d, "transforms", f"{i}.json"), "w") as fh:
                json.dump({"transforms": ts}, fh)
        with open(os.path.join(d, "labels.txt"), "w") as fh:
            fh.write("".join(f"l{i}.nii.gz\n" for i in range(n)))
        extent = [(N - 1) * s[0], (N - 1) * s[1], (args.depth - 1) * s[2]]
        with open(os.path.join(d, "bbox.json"), "w") as fh:
            json.dump({"bbox": [[0.0, 0.0, 0.0], extent]}, fh)
        out = {"images": n, "radius": args.radius}
        for key, extra in (("vote", []), ("joint", ["-j", "1"])):
            t0 = time.perf_counter()
            r = subprocess.run([os.path.join(ROOT, "bin", "AtlasSegment"), "bbox.json", repr(s[0]), "target.nii.gz"] + names +
                               ["-ll", "labels.txt", "-o", key, "-r", str(args.radius)] + extra, cwd=d, capture_output=True, text=True, timeout=900)
            wall = time.perf_counter() - t0
            if r.returncode != 0:
                raise RuntimeError(r.stdout[-2000:] + r.stderr[-2000:])
            grid = re.search(r"grid (\d+) x (\d+) x (\d+)", r.stdout)
            out[key] = {"wall_s": round(wall, 3), "grid_dims": [int(g) for g in grid.groups()] if grid else None,
                        "phases_s": {k: float(v) for k, v in re.findall(r"^(read|device|write|total) : ([0-9.]+) s", r.stdout, re.M)}}
        print(json.dumps(out))
    finally:
        shutil.rmtree(d, ignore_errors=True)


def merge(directory, out):
    kernels = {}
    for f in glob.glob(os.path.join(directory, "**", "*_kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "jlabels_" in r["Kernel_Name"] or "wlabels_" in r["Kernel_Name"]:
                kernels.setdefault(short(r["Kernel_Name"]), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    if kernels:
        out["kernels_under_rocprofv3"] = {k: {"launches": len(t), "mean_ms": round(float(np.mean(t)), 4), "min_ms": round(min(t), 4),
                                              "max_ms": round(max(t), 4)} for k, t in sorted(kernels.items())}
        solve = [k for k in kernels if "jlabels_solve" in k]
        if solve and "gram_f64_operations" in out and os.path.exists(os.path.join(directory, "trace_depth")):
            depth = int(open(os.path.join(directory, "trace_depth")).read())
            ops = gram_operations((N, N, depth), out["images"], out["radius"])
            rate = ops / (sum(kernels[solve[0]]) * 1e-3)
            out["solve_kernel"] = {"grid": [N, N, depth], "gram_f64_operations": ops, "ms": round(sum(kernels[solve[0]]), 3),
                                   "gram_operations_per_s": round(rate, 1), "of_vector_f64_rate": round(rate / F64_OPS_PER_S, 4),
                                   "vector_f64_operations_per_s": F64_OPS_PER_S}
    counters = collections.defaultdict(lambda: collections.defaultdict(lambda: [0.0, 0]))
    for f in glob.glob(os.path.join(directory, "**", "*_counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "jlabels_solve" in r["Kernel_Name"]:
                c = counters[short(r["Kernel_Name"])][r["Counter_Name"]]
                c[0] += float(r["Counter_Value"]); c[1] += 1
    if counters:
        out["solve_kernel_counters_per_launch"] = {k: {name: round(v / m, 1) for name, (v, m) in sorted(c.items())} for k, c in sorted(counters.items())}
    for name, key in (("tool.json", "atlas_segment_tool"), ("pmc_depth", "counters_grid_depth")):
        path = os.path.join(directory, name)
        if os.path.exists(path):
            out[key] = json.loads(open(path).read())
    ab_lines = os.path.join(directory, "ab.jsonl")             # profile_jlabels.sh's second argument: --ab runs in turn
    if os.path.exists(ab_lines):
        out["adds_and_reslice_by_library_in_turn"] = [json.loads(line) for line in open(ab_lines) if line.strip()]
    return out


def ab(args):
    """frog_labels_add, frog_wlabels_add and frog_chain_reslice through args.ab, by ctypes alone."""
    from frog_amd import _abi
    lib = C.CDLL(os.path.abspath(args.ab))
    for name in ("frog_chain_create", "frog_chain_destroy", "frog_chain_invert_links", "frog_chain_reslice", "frog_labels_create", "frog_labels_add",
                 "frog_labels_destroy", "frog_wlabels_create", "frog_wlabels_target", "frog_wlabels_add", "frog_wlabels_destroy"):
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
    t_add, t_wadd, t_reslice = [], [], []
    for rep in range(args.repeats + 1):
        acc, wacc = C.c_void_p(), C.c_void_p()
        assert lib.frog_labels_create(C.byref(grid), 8, 0, 0, C.byref(acc)) == 0
        assert lib.frog_wlabels_create(C.byref(grid), 8, 0, 2, 2, 2.0 ** -10, 0, C.byref(wacc)) == 0
        assert lib.frog_wlabels_target(wacc, chain, C.byref(iv), 1, 0.0, None) == 0
        for k in range(8):
            rc, ms = timed(lambda: lib.frog_labels_add(acc, chain, C.byref(lv), 0.0, None))
            assert rc == 0
            if rep and k:
                t_add.append(ms)
            rc, ms = timed(lambda: lib.frog_wlabels_add(wacc, chain, C.byref(iv), C.byref(lv), 1, 0.0, 0.0, None, None))
            assert rc == 0
            if rep and k:
                t_wadd.append(ms)
            rc, ms = timed(lambda: lib.frog_chain_reslice(chain, C.byref(iv), C.byref(ov), 1, 0.0))
            assert rc == 0
            if rep:
                t_reslice.append(ms)
        lib.frog_labels_destroy(acc)
        lib.frog_wlabels_destroy(wacc)
    lib.frog_chain_destroy(chain)
    print(json.dumps({"library": args.ab, "labels_add": stats(t_add), "wlabels_add": stats(t_wadd), "chain_reslice": stats(t_reslice)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "joint_fusion.json"))
    ap.add_argument("--images", type=int, default=20)
    ap.add_argument("--radius", type=int, default=2)
    ap.add_argument("--depth", type=int, default=N)
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--tool", action="store_true")
    ap.add_argument("--merge")
    ap.add_argument("--ab")
    args = ap.parse_args()
    if args.trace_run:
        return trace_run(args)
    if args.tool:
        return tool(args)
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
