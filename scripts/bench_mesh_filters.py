#!/usr/bin/env python3
"""The mesh filters at volume size: the two surfaces of scripts/bench_isosurface.py on the 256^3 grid, the uint16
label surface and the float32 probability map's, smoothed and clustered on the device where frog_isosurface_create left them.

  bench_mesh_filters.py [--out FILE]   wall times, the median of 5 whole calls (host clock; every call ends in a synchronisation):
                                       frog_isosurface_smooth at 1 iteration (the adjacency build and two passes) and at 20, in
                                       child processes with 16-byte (FROG_MESH_STRIDE=4) and 12-byte (=3) working rows;
                                       frog_isosurface_cluster at a cell of two voxels; bin/IsoSurface -s 20 -c ... against plain
                                       bin/IsoSurface end to end
  bench_mesh_filters.py --trace-run    per surface two rounds of create, smooth 20, cluster, nothing else: the command to run
                                       under `rocprofv3 --kernel-trace --stats -d DIR -o p --output-format csv`, once per
                                       FROG_MESH_STRIDE
  bench_mesh_filters.py --merge DIR [--key NAME]
                                       reads DIR's kernel trace (no device needed) and sets the adjacency build's, the pass
                                       kernel's and the clustering's times under NAME, the pass kernel beside the bytes it must
                                       move at the device's measured streaming rate"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_isosurface import HBM_BYTES_PER_S, Surface, cases, probability_volume       # noqa: E402
from bench_labels import GRID, N, stats, timed                                           # noqa: E402

CELL = 2 * 400.0 / 256              # two voxels
ITERATIONS, LAM, MU = 20, 0.5, -0.53


def smooth(s, iterations):
    s.abi.check(s.lib.frog_isosurface_smooth(s.h, iterations, LAM, MU, 1), "smooth")


def cluster(s):
    n, m = C.c_uint32(), C.c_uint32()
    s.abi.check(s.lib.frog_isosurface_cluster(s.h, CELL, C.byref(n), C.byref(m), None), "cluster")
    return n.value, m.value


def csr_entries(n, tri):
    """The number of entries of the passes' CSR (boundary = 1), as include/frog_chain.h defines N(v)."""
    t = tri.astype(np.int64)
    a = np.concatenate([t[:, 0], t[:, 1], t[:, 2]])
    b = np.concatenate([t[:, 1], t[:, 2], t[:, 0]])
    keep = a != b
    a, b = a[keep], b[keep]
    unique, times = np.unique(np.concatenate([a << 32 | b, b << 32 | a]), return_counts=True)
    row = unique >> 32
    on_boundary = np.zeros(n, bool)
    on_boundary[row[times == 1]] = True
    return int((~on_boundary[row] | (times == 1)).sum())


def smooth_times(repeats):
    """Per case the wall times of frog_isosurface_smooth at 1 and at 20 iterations, each on a fresh surface."""
    res = {}
    for name, (volume, how) in cases().items():
        t1, t20 = [], []
        for rep in range(repeats + 1):                      # the first round warms up
            for iterations, into in ((1, t1), (ITERATIONS, t20)):
                s = Surface(volume, **how)
                ms = timed(lambda: smooth(s, iterations))[1]
                s.close()
                if rep:
                    into.append(ms)
        res[name] = {"smooth_1_iteration": stats(t1), "smooth_20_iterations": stats(t20)}
    return res


def measure(args):
    out = {"what": "scripts/bench_mesh_filters.py on one MI355X: the two surfaces of scripts/bench_isosurface.py (256^3 grid at 400/256 mm), "
                   "frog_isosurface_smooth with lambda %.2f, mu %.2f, boundary 1 and frog_isosurface_cluster at a cell of two voxels "
                   "(%.4f mm); wall times are host-clock times of whole calls" % (LAM, MU, CELL),
           "cases": {}}
    rows = {}
    for stride in ("4", "3"):                               # the switch is read once per process
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--smooth-only", "--repeats", str(args.repeats)],
                               env=dict(os.environ, FROG_MESH_STRIDE=stride), capture_output=True, text=True, timeout=900)
        if child.returncode != 0:
            raise RuntimeError(child.stdout[-2000:] + child.stderr[-2000:])
        rows[stride] = json.loads(child.stdout)
    padded, packed = rows["4"], rows["3"]
    for name, (volume, how) in cases().items():
        t_cluster = []
        for rep in range(args.repeats + 1):
            s = Surface(volume, **how)
            n0, m0 = s.n, s.m
            if rep == 0:
                entries = csr_entries(s.n, s.get()[1])
            smooth(s, ITERATIONS)
            (n1, m1), ms = timed(lambda: cluster(s))
            s.close()
            if rep:
                t_cluster.append(ms)
        out["cases"][name] = {"vertices": n0, "triangles": m0, "csr_entries": entries, "clustered_vertices": n1, "clustered_triangles": m1,
                              "wall": {"rows_of_16_bytes": padded[name], "rows_of_12_bytes": packed[name], "isosurface_cluster": stats(t_cluster)}}
        print(name, "done", file=sys.stderr, flush=True)
    out["tools"] = tools()
    return out


def tools():
    """bin/IsoSurface on the probability map as an uncompressed .nii: plain, and with -s 20 -c."""
    from frog_amd.volume import write_volume
    d = tempfile.mkdtemp(prefix="bench_mesh_")
    try:
        write_volume(os.path.join(d, "p.nii"), probability_volume(), GRID[1], GRID[2])
        res = {}
        for name, cmd in (("IsoSurface_level_to_ply", ["IsoSurface", "p.nii", "-l", "0.5", "-o", "s.ply"]),
                          ("IsoSurface_level_smoothed_clustered_to_ply", ["IsoSurface", "p.nii", "-l", "0.5", "-s", str(ITERATIONS), "-c", str(CELL), "-o", "f.ply"]),
                          ("IsoSurface_level_to_obj", ["IsoSurface", "p.nii", "-l", "0.5", "-o", "s.obj"]),
                          ("IsoSurface_level_smoothed_clustered_to_obj", ["IsoSurface", "p.nii", "-l", "0.5", "-s", str(ITERATIONS), "-c", str(CELL), "-o", "f.obj"])):
            walls = []
            for _ in range(3):
                t0 = time.perf_counter()
                r = subprocess.run([os.path.join(ROOT, "bin", cmd[0])] + cmd[1:], cwd=d, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise RuntimeError(r.stdout[-2000:] + r.stderr[-2000:])
                walls.append(time.perf_counter() - t0)
            res[name] = {"wall_s_median_of_3": round(sorted(walls)[1], 3), "output_bytes": os.path.getsize(os.path.join(d, cmd[-1]))}
        return res
    finally:
        shutil.rmtree(d, ignore_errors=True)


def trace_run(args):
    for name, (volume, how) in cases().items():
        for _ in range(2):
            s = Surface(volume, **how)
            smooth(s, ITERATIONS)
            cluster(s)
            s.close()


def merge(directory, out, key):
    files = glob.glob(os.path.join(directory, "**", "*_kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"one *_kernel_trace.csv expected under {directory}, found {len(files)}")
    rows = [(r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0],
             (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
            for r in sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))]
    # trace_run: per case two rounds; a round begins with iso_classify_kernel and the second round is the warm one
    rounds = []
    for name, ms in rows:
        if name.startswith("iso_classify_kernel"):
            rounds.append([])
        if rounds:
            rounds[-1].append((name, ms))
    for k, case in enumerate(out["cases"]):
        c = out["cases"][case]
        if len(rounds) <= 2 * k + 1:
            continue
        warm = rounds[2 * k + 1]
        names = [name for name, _ in warm]
        last_iso = max(i for i, name in enumerate(names) if name.startswith("iso_"))
        first_pass = next((i for i, name in enumerate(names) if name.startswith(("mesh_pass_kernel", "mesh_pad_kernel"))), len(warm))
        first_cluster = next((i for i, name in enumerate(names) if name.startswith("mesh_bounds_kernel")), len(warm))
        passes = [ms for name, ms in warm if name.startswith("mesh_pass_kernel")]
        build = [ms for _, ms in warm[last_iso + 1:first_pass]]       # the key kernel, the sort, the run lengths, rows, degrees, scan, fill
        clustering = [ms for name, ms in warm[first_cluster:]]
        must = 4 * (c["vertices"] + 1) + 4 * c["csr_entries"] + 24 * c["vertices"]
        kernels = {"adjacency_build_all_kernels_ms": round(sum(build), 4), "adjacency_build_launches": len(build),
                   "cluster_all_kernels_ms": round(sum(clustering), 4), "cluster_launches": len(clustering)}
        if passes:
            median = float(np.median(passes))
            kernels["mesh_pass_kernel"] = {"launches": len(passes), "median_ms": round(median, 4), "min_ms": round(min(passes), 4),
                                           "max_ms": round(max(passes), 4), "must_move_bytes": must,
                                           "at_hbm_rate_ms": round(must / HBM_BYTES_PER_S * 1e3, 4),
                                           "times_the_bound": round(median / (must / HBM_BYTES_PER_S * 1e3), 2),
                                           "gathered_bytes_16_per_entry": 16 * c["csr_entries"]}
        c[key] = kernels
    out["hbm_bytes_per_s"] = HBM_BYTES_PER_S


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_filters.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--smooth-only", action="store_true", help="print smooth_times() as JSON (the children under FROG_MESH_STRIDE)")
    ap.add_argument("--merge")
    ap.add_argument("--key", default="kernels_under_rocprofv3_rows_of_16_bytes")
    args = ap.parse_args()
    if args.trace_run:
        return trace_run(args)
    if args.smooth_only:
        print(json.dumps(smooth_times(args.repeats)))
        return
    if args.merge:
        out = json.load(open(args.out))
        merge(args.merge, out, args.key)
    else:
        out = measure(args)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
