#!/usr/bin/env python3
"""frog_labels at volume size: the 256^3 grid and the 1 + 7 link chain of scripts/bench_field.py (one seeded
chain per image, inverted), 20 uint16 label images of 256^3 voxels that carry 20 RadLex-like values in blocks.

  bench_labels.py [--out FILE]        wall times (host clock around whole calls; every call ends in a synchronisation or a
                                      device-to-host copy): per frog_labels_add, beside frog_average_add(interpolation 0) on
                                      the same volume and chain in the same process, alternating; finish, table, fused,
                                      probability; then bin/FuseLabels on the same inputs as files, for its phase lines
  bench_labels.py --trace-run         one accumulation and every getter once, nothing else: the command to run under
                                      `rocprofv3 --kernel-trace --stats -d DIR -o p --output-format csv`
  bench_labels.py --merge DIR         reads DIR's kernel trace (no device needed) and adds the kernel times
The finish-side kernels read n_labels x voxels x 2 bytes of counts; their times are set beside that."""
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

N = 256
GRID = ((N, N, N), (0.0, 0.0, 0.0), (400 / N,) * 3)         # dims, origin, spacing
VALUES = np.array([0, 58, 86, 170, 237, 480, 1247, 1302, 1326, 2473, 7578, 29193, 29662, 29663, 30324, 30325, 32248, 32249, 40357, 40358],
                  np.uint16)
PEAK_BYTES_PER_S = 8e12                                     # the peak DESIGN.md's streaming-kernel rows divide by


def chain_links(seed, amplitude=1.0):
    from frog_amd.chain import Link
    rng = np.random.default_rng(seed)
    M = np.eye(4); M[:3, 3] = rng.uniform(-3, 3, 3)
    links = [Link.linear(M)]
    for n in (4, 4, 8, 8, 16, 16, 16):
        dims = (n + 3, n + 3, n + 3)
        sp = tuple(400.0 / n for _ in range(3))
        links.append(Link.bspline(dims, tuple(-s for s in sp), sp, (amplitude * rng.normal(size=(dims[0] ** 3, 3))).astype(np.float32)))
    return links


def label_volume(image):
    """Blocks of 40 x 48 x 56 voxels, shifted per image, numbered onto the 20 values."""
    z, y, x = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij", sparse=True)
    block = ((x + 3 * image) // 40 + 3 * ((y + 2 * image) // 48) + 7 * ((z + image) // 56)) % len(VALUES)
    return VALUES[block]


def stats(t):
    return {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(min(t)), 3), "count": len(t)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def streamed(n_labels, ms):
    b = n_labels * N ** 3 * 2
    return {"count_bytes": b, "bytes_per_s": round(b / (ms * 1e-3), 1), "of_8_TB_per_s": round(b / (ms * 1e-3) / PEAK_BYTES_PER_S, 4)}


def measure(args):
    from frog_amd.chain import Chain, invert
    from frog_amd.volume import Average, Labels
    n = args.images
    o, s = GRID[1], GRID[2]
    vols = [(label_volume(i), o, s) for i in range(n)]
    chains = [Chain(invert(chain_links(100 + i))) for i in range(n)]
    out = {"what": "scripts/bench_labels.py on one MI355X: %d uint16 label images of 256^3 voxels with %d values, each through the "
                   "inverse of 1 matrix + 7 lattices (4, 4, 8, 8, 16, 16, 16 cells over 400 mm) onto a 256^3 grid at 400/256 mm; "
                   "wall times are host-clock times of whole calls, copies included" % (n, len(VALUES)),
           "images": n, "voxels": N ** 3, "wall": {}}
    w = out["wall"]
    t_labels, t_average, t_finish, t_table, t_fused, t_prob = [], [], [], [], [], []
    for rep in range(args.repeats + 1):                     # the first round warms up (code objects, first allocations)
        acc, avg = Labels(GRID, n), Average(GRID, n)
        tl, ta = [], []
        for v, c in zip(vols, chains):
            tl.append(timed(lambda: acc.add(v, c, 0.0))[1])
            ta.append(timed(lambda: avg.add(v, c, 0, 0.0))[1])
        n_labels, ms_finish = timed(acc.finish)
        table, ms_table = timed(acc.table)
        (fused, agreement), ms_fused = timed(acc.fused)
        _, ms_prob = timed(lambda: acc.probability(int(table[0][0])))
        avg.finish()
        acc.close(); avg.close()
        if rep:
            t_labels += tl[1:]; t_average += ta[1:]          # the first add of an accumulator allocates the label planes
            t_finish.append(ms_finish); t_table.append(ms_table); t_fused.append(ms_fused); t_prob.append(ms_prob)
            w.setdefault("labels_add_first_ms", []).append(round(tl[0], 3))
    w["labels_add"], w["average_add_nearest"] = stats(t_labels), stats(t_average)
    w["labels_add_over_average_add"] = round(w["labels_add"]["median_ms"] / w["average_add_nearest"]["median_ms"], 3)
    w["finish"], w["table"], w["fused"], w["probability"] = stats(t_finish), stats(t_table), stats(t_fused), stats(t_prob)
    out["n_labels"] = n_labels
    out["fused_dtype"] = str(fused.dtype)
    out["mean_agreement"] = round(float(agreement.mean()), 4)
    out["finish_streams"] = streamed(n_labels, w["finish"]["median_ms"])
    out["tool"] = tool(args, vols)
    return out


def tool(args, vols):
    """bin/FuseLabels on the same images and chains as files: its phase lines."""
    from frog_amd.volume import write_volume
    d = tempfile.mkdtemp(prefix="bench_labels_")
    try:
        os.makedirs(os.path.join(d, "transforms"))
        names = []
        for i, (v, o, s) in enumerate(vols):
            names.append(f"l{i}.nii.gz")
            write_volume(os.path.join(d, names[-1]), v, o, s)
            ts = []
            for l in chain_links(100 + i):
                if l.matrix is not None:
                    ts.append({"type": "vtkMatrixToLinearTransform", "matrix": l.matrix.ravel().tolist()})
                else:
                    ts.append({"type": "vtkBSplineTransform", "dimensions": list(l.dims), "origin": list(l.origin), "spacing": list(l.spacing),
                               "coeffs": [float(c) for c in l.coeffs.ravel()]})
            with open(os.path.join(d, "transforms", f"{i}.json"), "w") as fh:
                json.dump({"transforms": ts}, fh)
        extent = [(N - 1) * s for s in GRID[2]]
        with open(os.path.join(d, "bbox.json"), "w") as fh:
            json.dump({"bbox": [[0.0, 0.0, 0.0], extent]}, fh)
        t0 = time.perf_counter()
        r = subprocess.run([os.path.join(ROOT, "bin", "FuseLabels"), "bbox.json", repr(GRID[2][0])] + names + ["-o", "out"], cwd=d,
                           capture_output=True, text=True, timeout=600)
        wall = time.perf_counter() - t0
        if r.returncode != 0:
            raise RuntimeError(r.stdout[-2000:] + r.stderr[-2000:])
        phases = {k: float(v) for k, v in re.findall(r"^(read|device|write|total) : ([0-9.]+) s", r.stdout, re.M)}
        grid = re.search(r"grid (\d+) x (\d+) x (\d+)", r.stdout)
        setup = re.search(r"\(\+ ([0-9.]+) s set-up\)", r.stdout)
        waited = re.search(r"\(device waited ([0-9.]+) s\)", r.stdout)
        return {"wall_s": round(wall, 3), "grid_dims": [int(g) for g in grid.groups()], "phases_s": phases,
                "device_setup_s": float(setup.group(1)), "device_waited_for_read_s": float(waited.group(1))}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def trace_run(args):
    from frog_amd.chain import Chain, invert
    from frog_amd.volume import Average, Labels
    n = args.images
    acc, avg = Labels(GRID, n), Average(GRID, n)
    for i in range(n):
        v, c = (label_volume(i), GRID[1], GRID[2]), Chain(invert(chain_links(100 + i)))
        acc.add(v, c, 0.0)
        avg.add(v, c, 0, 0.0)
        c.close()
    acc.finish()
    acc.fused()
    acc.probability(0)
    avg.finish()


def merge(directory, out):
    files = glob.glob(os.path.join(directory, "**", "*_kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"one *_kernel_trace.csv expected under {directory}, found {len(files)}")
    kernels = {}
    for r in csv.DictReader(open(files[0])):
        name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        if "labels_" in name or "reslice_accumulate" in name:
            kernels.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    out["kernels_under_rocprofv3"] = {k: {"launches": len(t), "mean_ms": round(float(np.mean(t)), 4), "min_ms": round(min(t), 4),
                                          "max_ms": round(max(t), 4)} for k, t in sorted(kernels.items())}
    n_labels = out.get("n_labels", len(VALUES))
    for k, t in kernels.items():
        if "labels_table" in k or "labels_fused" in k:
            out["kernels_under_rocprofv3"][k]["counts_read"] = streamed(n_labels, float(np.mean(t)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "label_fusion.json"))
    ap.add_argument("--images", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=2)
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
