#!/usr/bin/env python3
"""frog_surface at volume size: scripts/bench_labels.py's case -- a 256^3 grid, 20 uint16 label images with 20
RadLex-like values in blocks, one seeded 1 + 7 link chain per image.  The reference is the group's majority vote and the 19
values other than the background are measured.

  bench_surface.py [--out FILE]       wall times (host clock around whole calls, each of which ends in a device-to-host copy):
                                      frog_surface_create; per frog_surface_add, beside frog_labels_add on the same volume
                                      and chain in the same process, in turn -- both pay the same chain evaluation, so the
                                      difference is what the distances cost; frog_distance_map of one label on the whole grid;
                                      then bin/FuseLabels on the same inputs as files, without and with -d 1
  bench_surface.py --trace-run        one create and one add per image, nothing else: the command to run under
                                      `rocprofv3 --kernel-trace --stats -d DIR -o p --output-format csv`
  bench_surface.py --merge DIR        reads DIR's kernel trace (no device needed) and adds the kernel times.  The create runs
                                      the three passes once per value over the whole grid, so the first `n_values` launches of
                                      edt_x_kernel and edt_y_kernel (and every edt_z_kernel) are the passes without cropping;
                                      the later ones, and edt_z_collect_kernel, are the adds' cropped passes."""
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_labels import GRID, N, VALUES, chain_links, label_volume, stats, timed  # noqa: E402

MEASURED = [int(v) for v in VALUES if v != 0]


def group(n):
    from frog_amd.chain import Chain, invert
    o, s = GRID[1], GRID[2]
    return [(label_volume(i), o, s) for i in range(n)], [Chain(invert(chain_links(100 + i))) for i in range(n)]


def vote(vols, chains):
    """The majority vote of the group (the reference) and the wall time of every frog_labels_add."""
    from frog_amd.volume import Labels
    acc = Labels(GRID, len(vols))
    times = [timed(lambda: acc.add(v, c, 0.0))[1] for v, c in zip(vols, chains)]
    acc.finish()
    labels, _ = acc.fused()
    acc.close()
    return labels, times


def measure(args):
    from frog_amd.volume import Labels, SurfaceDistances, distance_map, surface_metrics
    n = args.images
    vols, chains = group(n)
    out = {"what": "scripts/bench_surface.py on one MI355X: %d uint16 label images of 256^3 voxels with %d values, each through the "
                   "inverse of 1 matrix + 7 lattices onto a 256^3 grid at 400/256 mm, against their majority vote, %d values "
                   "measured; wall times are host-clock times of whole calls, copies included" % (n, len(VALUES), len(MEASURED)),
           "images": n, "voxels": N ** 3, "n_values": len(MEASURED), "wall": {}}
    w = out["wall"]
    reference, _ = vote(vols, chains)
    t_create, t_surface, t_labels, t_map = [], [], [], []
    for rep in range(args.repeats + 1):                     # the first round warms up (code objects, first allocations)
        sd, ms_create = timed(lambda: SurfaceDistances(reference, MEASURED, GRID))
        lab = Labels(GRID, n)
        ts, tl, rows = [], [], []
        for v, c in zip(vols, chains):
            r, ms = timed(lambda: sd.add(v, c, 0.0))
            ts.append(ms); rows.append(r)
            tl.append(timed(lambda: lab.add(v, c, 0.0))[1])
        sd.close(); lab.close()
        _, ms_map = timed(lambda: distance_map(reference, MEASURED[0], GRID[2], 1))
        if rep:
            t_create.append(ms_create); t_map.append(ms_map)
            t_surface += ts[1:]; t_labels += tl[1:]          # the first add of an accumulator allocates
    w["surface_create"], w["surface_add"], w["labels_add"] = stats(t_create), stats(t_surface), stats(t_labels)
    w["distance_map_whole_grid"] = stats(t_map)
    w["surface_add_over_labels_add"] = round(w["surface_add"]["median_ms"] / w["labels_add"]["median_ms"], 3)
    hausdorff, hausdorff_p, assd = surface_metrics(np.stack(rows))
    surface = np.stack(rows)["n_a"].sum(1)
    out["surface_voxels_per_image"] = {"median": int(np.median(surface)), "share_of_grid": round(float(np.median(surface)) / N ** 3, 4)}
    out["mean_assd_mm"] = round(float(np.nanmean(assd)), 4)
    out["max_hausdorff_mm"] = round(float(np.nanmax(hausdorff)), 4)
    out["tool"] = tool(vols)
    return out


def tool(vols):
    """bin/FuseLabels on the same images and chains as files, without and with -d 1: wall time and phase lines."""
    from frog_amd.volume import write_volume
    d = tempfile.mkdtemp(prefix="bench_surface_")
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
        with open(os.path.join(d, "bbox.json"), "w") as fh:
            json.dump({"bbox": [[0.0, 0.0, 0.0], [(N - 1) * s for s in GRID[2]]]}, fh)
        result = {}
        for key, extra in (("without", []), ("with_d_1", ["-d", "1"])):
            t0 = time.perf_counter()
            r = subprocess.run([os.path.join(ROOT, "bin", "FuseLabels"), "bbox.json", repr(GRID[2][0])] + names + ["-o", key] + extra, cwd=d,
                               capture_output=True, text=True, timeout=900)
            wall = time.perf_counter() - t0
            if r.returncode != 0:
                raise RuntimeError(r.stdout[-2000:] + r.stderr[-2000:])
            phases = {k: float(v) for k, v in re.findall(r"^(read|device|write|total|surface) : ([0-9.]+) s", r.stdout, re.M)}
            result[key] = {"wall_s": round(wall, 3), "phases_s": phases}
        return result
    finally:
        shutil.rmtree(d, ignore_errors=True)


def trace_run(args):
    from frog_amd.volume import SurfaceDistances
    vols, chains = group(args.images)
    reference, _ = vote(vols, chains)
    with SurfaceDistances(reference, MEASURED, GRID) as sd:
        for v, c in zip(vols, chains):
            sd.add(v, c, 0.0)


def merge(directory, out):
    files = glob.glob(os.path.join(directory, "**", "*_kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"one *_kernel_trace.csv expected under {directory}, found {len(files)}")
    launches = []
    for r in csv.DictReader(open(files[0])):
        name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].split("<")[0]
        if name.startswith("edt_") or "labels_" in name or name == "reslice_kernel":
            launches.append((int(r["Start_Timestamp"]), name, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
    launches.sort()
    whole = out.get("n_values", len(MEASURED))
    kernels, seen = {}, {}
    for _, name, ms in launches:
        seen[name] = seen.get(name, 0) + 1
        if name in ("edt_x_kernel", "edt_y_kernel"):
            name += " (whole grid)" if seen[name] <= whole else " (cropped)"
        elif name == "edt_z_kernel":
            name += " (whole grid)"
        elif name == "edt_z_collect_kernel":
            name += " (cropped, at the reference's surface)"
        kernels.setdefault(name, []).append(ms)
    table = {k: {"launches": len(t), "mean_ms": round(float(np.mean(t)), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                 "total_ms": round(float(np.sum(t)), 3)} for k, t in sorted(kernels.items())}
    n = out.get("images", 20)
    per_add = {k: round(v["total_ms"] / n, 3) for k, v in table.items() if "whole grid" not in k and not k.startswith("labels_")}
    out["kernels_under_rocprofv3"] = {"kernels": table, "surface_add_kernel_ms_per_image": per_add,
                                      "surface_add_kernel_ms_per_image_total": round(sum(per_add.values()), 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface.json"))
    ap.add_argument("--images", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=1)
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
