#!/usr/bin/env python3
"""frog_isosurface at volume size: the 256^3 grid of scripts/bench_labels.py; a uint16 label map (its image 0) in
label mode at one of its values, and a float32 probability map at 0.5 in level mode.

  bench_isosurface.py [--out FILE]    wall times (host clock around whole calls; every call ends in a synchronisation or a
                                      device-to-host copy): frog_isosurface_create whole, frog_isosurface_get, frog_isosurface_apply
                                      beside frog_chain_apply_f32 and frog_chain_apply on the same points (1 matrix + 7 lattices), and
                                      bin/IsoSurface and bin/MeshTransform end to end on the same inputs as files
  bench_isosurface.py --trace-run     both extractions and one apply, nothing else: the command to run under
                                      `rocprofv3 --kernel-trace --stats -d DIR -o p --output-format csv`
  bench_isosurface.py --merge DIR     reads DIR's kernel trace (no device needed) and sets each kernel's time beside the bytes
                                      it must move at the device's measured streaming rate"""
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

from bench_labels import GRID, N, VALUES, chain_links, label_volume, stats, timed         # noqa: E402

HBM_BYTES_PER_S = 6.29e12           # the measured streaming rate of the device (a float4 copy)
LABEL = int(VALUES[1])


def probability_volume():
    z, y, x = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij", sparse=True)
    return (0.5 + 0.5 * np.sin(x / 17.0) * np.sin(y / 19.0) * np.sin(z / 23.0)).astype(np.float32)


def cases():
    return {"label_u16": (label_volume(0), dict(label=LABEL)), "level_f32": (probability_volume(), dict(level=0.5))}


class Surface:
    """The handle by hand, so that create, apply and get are timed apart."""

    def __init__(self, volume, level=None, label=None):
        from frog_amd import _abi
        self.lib = _abi.hip_lib()
        self.abi = _abi
        v = _abi.volume_view(volume, GRID[1], GRID[2])
        self.h, n, m = C.c_void_p(), C.c_uint32(), C.c_uint32()
        _abi.check(self.lib.frog_isosurface_create(C.byref(v), int(label is not None), 0.0 if level is None else level,
                                                   0 if label is None else label, 0, C.byref(self.h), C.byref(n), C.byref(m)), "create")
        self.n, self.m = n.value, m.value

    def apply(self, chain):
        self.abi.check(self.lib.frog_isosurface_apply(self.h, chain._h), "apply")

    def get(self):
        xyz, tri = np.empty((self.n, 3), np.float32), np.empty((self.m, 3), np.uint32)
        self.abi.check(self.lib.frog_isosurface_get(self.h, xyz.ctypes.data_as(self.abi.c_float_p), tri.ctypes.data_as(self.abi.c_u32_p)), "get")
        return xyz, tri

    def close(self):
        self.lib.frog_isosurface_destroy(self.h)


def measure(args):
    from frog_amd.chain import Chain
    from frog_amd.mesh import transform_points
    chain = Chain(chain_links(100))
    out = {"what": "scripts/bench_isosurface.py on one MI355X: a 256^3 grid at 400/256 mm; label_u16 = the uint16 label map of "
                   "scripts/bench_labels.py (image 0) in label mode at %d, level_f32 = a float32 probability map at 0.5 in level mode; "
                   "the chain is 1 matrix + 7 lattices; wall times are host-clock times of whole calls, copies included" % LABEL,
           "nodes": N ** 3, "cases": {}}
    for name, (volume, how) in cases().items():
        t_create, t_get, t_apply, t_f32, t_f64 = [], [], [], [], []
        for rep in range(args.repeats + 1):                 # the first round warms up
            s, ms = timed(lambda: Surface(volume, **how))
            (xyz, tri), ms_get = timed(s.get)
            ms_apply = timed(lambda: s.apply(chain))[1]
            s.close()
            ms_f32 = timed(lambda: transform_points(chain, xyz))[1]
            ms_f64 = timed(lambda: chain.apply(xyz.astype(np.float64)))[1]
            if rep:
                t_create.append(ms); t_get.append(ms_get); t_apply.append(ms_apply); t_f32.append(ms_f32); t_f64.append(ms_f64)
        out["cases"][name] = {"dtype": str(volume.dtype), "vertices": s.n, "triangles": s.m, "volume_bytes": volume.nbytes,
                              "mesh_bytes": 12 * (s.n + s.m),
                              "wall": {"isosurface_create": stats(t_create), "isosurface_get": stats(t_get), "isosurface_apply": stats(t_apply),
                                       "chain_apply_f32_same_points": stats(t_f32), "chain_apply_f64_same_points": stats(t_f64)}}
        print(name, "done", file=sys.stderr, flush=True)
    out["tools"] = tools()
    return out


def tools():
    """bin/IsoSurface on the probability map as an uncompressed .nii, then bin/MeshTransform on its mesh."""
    from frog_amd.volume import write_volume
    d = tempfile.mkdtemp(prefix="bench_iso_")
    try:
        write_volume(os.path.join(d, "p.nii"), probability_volume(), GRID[1], GRID[2])
        ts = []
        for l in chain_links(100):
            if l.matrix is not None:
                ts.append({"type": "vtkMatrixToLinearTransform", "matrix": l.matrix.ravel().tolist()})
            else:
                ts.append({"type": "vtkBSplineTransform", "dimensions": list(l.dims), "origin": list(l.origin), "spacing": list(l.spacing),
                           "coeffs": [float(c) for c in l.coeffs.ravel()]})
        with open(os.path.join(d, "t.json"), "w") as fh:
            json.dump({"transforms": ts}, fh)
        res = {}
        for name, cmd in (("IsoSurface_level_to_ply", ["IsoSurface", "p.nii", "-l", "0.5", "-o", "s.ply"]),
                          ("IsoSurface_level_transformed_to_ply", ["IsoSurface", "p.nii", "-l", "0.5", "-t", "t.json", "-o", "st.ply"]),
                          ("MeshTransform_ply_to_ply", ["MeshTransform", "s.ply", "-t", "t.json", "-o", "m.ply"]),
                          ("MeshTransform_ply_to_obj", ["MeshTransform", "s.ply", "-t", "t.json", "-o", "m.obj"])):
            t0 = time.perf_counter()
            r = subprocess.run([os.path.join(ROOT, "bin", cmd[0])] + cmd[1:], cwd=d, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError(r.stdout[-2000:] + r.stderr[-2000:])
            res[name] = {"wall_s": round(time.perf_counter() - t0, 3), "output_bytes": os.path.getsize(os.path.join(d, cmd[-1]))}
        return res
    finally:
        shutil.rmtree(d, ignore_errors=True)


def trace_run(args):
    from frog_amd.chain import Chain
    chain = Chain(chain_links(100))
    for name, (volume, how) in cases().items():
        for _ in range(2):
            s = Surface(volume, **how)
            s.apply(chain)
            s.close()


def merge(directory, out):
    files = glob.glob(os.path.join(directory, "**", "*_kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"one *_kernel_trace.csv expected under {directory}, found {len(files)}")
    rows = [(r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0],
             (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
            for r in sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))]
    # trace_run: per case two rounds of classify, scans, vertices, triangles, apply; the second round is the warm one
    nodes = out["nodes"]
    order = list(out["cases"])
    seen = {}
    for name, ms in rows:
        if name.startswith(("iso_", "chain_apply_f32")):
            seen.setdefault(name, []).append(ms)
    scans = [ms for name, ms in rows if "scan" in name.lower() or "lookback" in name.lower()]
    for k, case in enumerate(order):
        c = out["cases"][case]
        size = c["volume_bytes"] // nodes
        typed = {"uint16": "unsigned short", "float32": "float"}[c["dtype"]]
        must = {"iso_classify_kernel<%s>" % typed: nodes * size + 2 * nodes,                 # the volume in, mask and configuration out
                "iso_vertices_kernel<%s>" % typed: nodes + 4 * nodes + 12 * c["vertices"],   # mask in, vertex_offset and vertices out
                "iso_triangles_kernel": nodes + 4 * nodes + nodes + 12 * c["triangles"]}      # configuration, vertex_offset, mask in, triangles out
        def warm(name):                                     # the second round's launch: typed kernels run for one case only
            t = seen.get(name, [])
            i = 1 if "<" in name else 2 * k + 1
            return t[i] if len(t) > i else None

        kernels = {}
        for name, b in must.items():
            if warm(name) is not None:
                kernels[name] = {"ms": round(warm(name), 4), "must_move_bytes": b, "at_hbm_rate_ms": round(b / HBM_BYTES_PER_S * 1e3, 4),
                                 "times_the_bound": round(warm(name) / (b / HBM_BYTES_PER_S * 1e3), 2)}
        if warm("chain_apply_f32_kernel") is not None:
            kernels["chain_apply_f32_kernel"] = {"ms": round(warm("chain_apply_f32_kernel"), 4), "points": c["vertices"]}
        c["kernels_under_rocprofv3"] = kernels
    out["scan_kernels_under_rocprofv3"] = {"launches": len(scans), "total_ms": round(sum(scans), 4),
                                           "per_create_ms": round(sum(scans) / max(1, 2 * len(order)), 4)}
    out["hbm_bytes_per_s"] = HBM_BYTES_PER_S


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "isosurface.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--merge")
    args = ap.parse_args()
    if args.trace_run:
        return trace_run(args)
    if args.merge:
        out = json.load(open(args.out))
        merge(args.merge, out)
    else:
        out = measure(args)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
