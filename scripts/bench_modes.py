#!/usr/bin/env python3
"""frog_modes at volume size: the 256^3 grid and the 1 + 7 link chains of scripts/bench_labels.py, 20 images, the
displacement as the value (3 components).

  bench_modes.py [--out FILE]         wall times (host clock around whole calls; every call ends in a synchronisation):
                                      frog_modes_add_displacement next to frog_chain_sample (displacement only, f32) on the same
                                      chain; frog_modes_gram with its folds, the median of 5; frog_modes_project for 8 modes (its
                                      nine fields copied to the host); bin/GroupModes -k 2 end to end with and without -ms 2
  bench_modes.py --trace-run          the adds, two grams and one projection, nothing else: the command to run under
                                      `rocprofv3 --kernel-trace --stats -d DIR -o p --output-format csv`
  bench_modes.py --merge DIR          reads DIR's kernel trace (no device needed) and adds the kernel times and the two
                                      yardsticks: the stored bytes at the HBM rate, the products and sums at the f64 rate"""
import argparse
import csv
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_labels import GRID, N, chain_links, stats, timed         # noqa: E402

IMAGES, DISTINCT, COMPONENTS, MODES, TILE = 20, 4, 3, 8, 32
F64_OPS_PER_S = 3.93e13             # the measured rate of separately rounded f64 operations
HBM_BYTES_PER_S = 6.29e12           # the measured streaming rate of the device (a float4 copy)


def filled(chains, times=None):
    from frog_amd.volume import ModeImages
    acc = ModeImages(GRID, IMAGES, COMPONENTS)
    for i in range(IMAGES):
        ms = timed(lambda: acc.add_displacement(chains[i % DISTINCT]))[1]
        if times is not None and i:
            times.append(ms)
    return acc


def weights():
    return np.random.default_rng(1).normal(size=(MODES, IMAGES)) / np.sqrt(IMAGES - 1.0)


def measure(args):
    from frog_amd.chain import Chain, invert
    chains = [Chain(invert(chain_links(100 + i))) for i in range(DISTINCT)]
    values = COMPONENTS * N ** 3
    out = {"what": "scripts/bench_modes.py on one MI355X: %d images (%d distinct chains of 1 matrix + 7 lattices, inverted, in turn) on a 256^3 "
                   "grid at 400/256 mm, value = displacement (3 components); wall times are host-clock times of whole calls, copies "
                   "included" % (IMAGES, DISTINCT),
           "voxels": N ** 3, "values_per_image": values, "stored_bytes": 4 * IMAGES * values, "pairs": IMAGES * (IMAGES + 1) // 2, "wall": {}}
    t_sample = [timed(lambda: chains[i % DISTINCT].sample(GRID[1], GRID[2], GRID[0], determinant=False))[1] for i in range(6)][1:]
    t_add = []
    acc = filled(chains, t_add)
    print("adds done", file=sys.stderr, flush=True)
    t_gram = [timed(lambda: acc.gram())[1] for _ in range(args.repeats + 1)][1:]
    out["n_support"] = acc.gram()[1]
    t_project = [timed(lambda: acc.project(weights()))[1] for _ in range(3)][1:]
    acc.close()
    w = out["wall"]
    w["chain_sample_displacement_f32"], w["modes_add_displacement"] = stats(t_sample), stats(t_add)
    w["modes_gram"], w["modes_project_8"] = stats(t_gram), stats(t_project)
    out["tool"] = {"plain": tool([]), "with_ms_2": tool(["-ms", "2"])}
    return out


def tool(extra):
    """bin/GroupModes -k 2 on the same chains as files: its phase lines."""
    d = tempfile.mkdtemp(prefix="bench_modes_")
    try:
        os.makedirs(os.path.join(d, "transforms"))
        for i in range(IMAGES):
            ts = []
            for l in chain_links(100 + i % DISTINCT):
                if l.matrix is not None:
                    ts.append({"type": "vtkMatrixToLinearTransform", "matrix": l.matrix.ravel().tolist()})
                else:
                    ts.append({"type": "vtkBSplineTransform", "dimensions": list(l.dims), "origin": list(l.origin), "spacing": list(l.spacing),
                               "coeffs": [float(c) for c in l.coeffs.ravel()]})
            with open(os.path.join(d, "transforms", f"{i}.json"), "w") as fh:
                json.dump({"transforms": ts}, fh)
        with open(os.path.join(d, "bbox.json"), "w") as fh:
            json.dump({"bbox": [[0.0, 0.0, 0.0], [(N - 1) * s for s in GRID[2]]]}, fh)
        t0 = time.perf_counter()
        r = subprocess.run([os.path.join(ROOT, "bin", "GroupModes"), "bbox.json", repr(GRID[2][0]), "-o", "out", "-k", "2"] + extra, cwd=d,
                           capture_output=True, text=True, timeout=900)
        wall = time.perf_counter() - t0
        if r.returncode != 0:
            raise RuntimeError(r.stdout[-2000:] + r.stderr[-2000:])
        phases = {k: float(v) for k, v in re.findall(r"^(read|device|write|total) : ([0-9.]+) s", r.stdout, re.M)}
        slabs = re.search(r"modes : (\d+) slab", r.stdout)
        return {"modes": 2, "fields_written": 3 + (5 if extra else 0), "wall_s": round(wall, 3), "slabs": int(slabs.group(1)), "phases_s": phases}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def trace_run(args):
    from frog_amd.chain import Chain, invert
    chains = [Chain(invert(chain_links(100 + i))) for i in range(DISTINCT)]
    chains[0].sample(GRID[1], GRID[2], GRID[0], determinant=False)
    acc = filled(chains)
    acc.gram()
    acc.gram()
    acc.project(weights())
    acc.close()


def executed_per_value():
    """The f64 multiplies and adds the Gram kernel issues per value: every wavefront with a thread that owns a 2 x 2 block of the
    lower triangle runs all 64 lanes (k_modes.hip.h)."""
    tiles = (IMAGES + TILE - 1) // TILE
    blocks = [(min(TILE, IMAGES - t * TILE) + 1) // 2 for t in range(tiles)]
    lanes = 0
    for i in range(tiles):
        for j in range(i + 1):
            owned = blocks[i] * (blocks[i] + 1) // 2 if i == j else blocks[i] * blocks[j]
            lanes += (owned + 63) // 64 * 64
    return 2 * 4 * lanes


def merge(directory, out):
    files = glob.glob(os.path.join(directory, "**", "*_kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"one *_kernel_trace.csv expected under {directory}, found {len(files)}")
    kernels = {}
    for r in sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"])):
        name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        if "modes_" in name or "chain_sample" in name:
            kernels.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    out["kernels_under_rocprofv3"] = {k: {"launches": len(t), "total_ms": round(sum(t), 4), "median_ms": round(float(np.median(t)), 4),
                                          "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)} for k, t in sorted(kernels.items())}

    def per_call(name, calls):
        t = [v for k, v in kernels.items() if k.startswith(name)]
        return sum(t[0]) / calls if t else None

    # trace_run calls gram twice and project once
    parts = {k: per_call(k, 2) for k in ("modes_mean_kernel", "modes_gram_kernel", "modes_fold_chunks_kernel", "modes_fold_planes_kernel")}
    if all(v is not None for v in parts.values()):
        tiles = (IMAGES + TILE - 1) // TILE
        read = out["stored_bytes"] * tiles + 8 * out["values_per_image"] * tiles * (tiles + 1) // 2     # each tile's values once per tile pair it is in, and the means
        ops = 2 * out["pairs"] * out["values_per_image"]
        ms = parts["modes_gram_kernel"]
        out["gram"] = {"kernels_ms_per_call": {k: round(v, 4) for k, v in parts.items()}, "all_kernels_ms": round(sum(parts.values()), 4),
                       "gram_kernel_bytes_read": read, "hbm_bound_ms": round(read / HBM_BYTES_PER_S * 1e3, 4),
                       "f64_operations_stated": ops, "f64_bound_ms": round(ops / F64_OPS_PER_S * 1e3, 4),
                       "f64_operations_executed": executed_per_value() * out["values_per_image"],
                       "gram_kernel_over_hbm_bound": round(ms / (read / HBM_BYTES_PER_S * 1e3), 2),
                       "gram_kernel_over_f64_bound": round(ms / (ops / F64_OPS_PER_S * 1e3), 2)}
    p = per_call("modes_project_kernel", 1)
    if p is not None:
        read = out["stored_bytes"] * 2                      # the mean's pass and the modes' pass
        out["project_8"] = {"kernel_ms": round(p, 4), "bytes": read + 4 * (MODES + 1) * out["values_per_image"],
                            "hbm_bound_ms": round((read + 4 * (MODES + 1) * out["values_per_image"]) / HBM_BYTES_PER_S * 1e3, 4),
                            "f64_bound_ms": round((2 * MODES + 2) * IMAGES * out["values_per_image"] / F64_OPS_PER_S * 1e3, 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_modes.json"))
    ap.add_argument("--repeats", type=int, default=5)
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
