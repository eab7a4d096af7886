#!/usr/bin/env python3
"""The group's average image two ways on the same inputs: bin/AverageImage (one process) against transform.sh's three-tool
flow (bin/DummyVolumeGenerator, one bin/VolumeTransform per image, bin/AverageVolumes).

Inputs are seeded and synthetic: N int16 volumes (.nii.gz) and transforms/<i>.json shaped like bin/frog's output (one
linear link, then one lattice per level, each level at half the previous spacing), a bbox.json over the volumes.  Both
flows must give the same average.nii.gz and stdev.nii.gz bit for bit.  Prints one JSON line: both wall times,
AverageImage's phase times and its device throughput in (image x grid voxel) / s.

    python scripts/bench_average.py [--images 20] [--dims 256 256 200] [--spacing 1.0] [--levels 3] [--workdir DIR]
"""
import argparse
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
from frog_amd.volume import read_volume, write_volume      # noqa: E402

BIN = os.path.join(ROOT, "bin")


def make_inputs(d, n_images, dims, levels, seed):
    """volumes v<i>.nii.gz (1 mm voxels, origin 0), transforms/<i>.json, bbox.json = the volumes' box"""
    rng = np.random.default_rng(seed)
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz, dtype=np.float32), np.arange(ny, dtype=np.float32), np.arange(nx, dtype=np.float32), indexing="ij")
    base = 900 + 500 * np.sin(x / 11.0) * np.cos(y / 13.0) + 2 * z
    extent = np.array(dims, np.float64)
    os.makedirs(os.path.join(d, "transforms"), exist_ok=True)
    names = []
    for i in range(n_images):
        v = (base + 30 * i + rng.normal(0, 20, base.shape).astype(np.float32)).astype(np.int16)
        names.append(f"v{i}.nii.gz")
        write_volume(os.path.join(d, names[-1]), v, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
        A = np.eye(3) + rng.normal(0, 0.02, (3, 3))
        M = np.eye(4); M[:3, :3] = A; M[:3, 3] = rng.uniform(-4, 4, 3) + (np.eye(3) - A) @ (extent / 2)
        ts = [{"type": "vtkMatrixToLinearTransform", "matrix": M.ravel().tolist()}]
        for level in range(levels):
            sp = 100.0 / 2 ** level
            ld = [int(np.ceil(e / sp)) + 3 for e in extent]
            co = (0.04 * sp * rng.normal(size=(ld[0] * ld[1] * ld[2], 3))).astype(np.float32)
            ts.append({"type": "vtkBSplineTransform", "dimensions": ld, "origin": [-sp] * 3, "spacing": [sp] * 3,
                       "coeffs": [float(c) for c in co.ravel()]})
        with open(os.path.join(d, "transforms", f"{i}.json"), "w") as fh:
            json.dump({"transforms": ts}, fh)
    with open(os.path.join(d, "bbox.json"), "w") as fh:
        json.dump({"bbox": [[0.0, 0.0, 0.0], [float(e) - 1 for e in extent]]}, fh)
    return names


def run(args, cwd):
    r = subprocess.run(args, cwd=cwd, capture_output=True, text=True, timeout=1200)
    if r.returncode != 0:
        sys.exit(f"{' '.join(args)} failed ({r.returncode}):\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=20)
    ap.add_argument("--dims", type=int, nargs=3, default=(256, 256, 200))
    ap.add_argument("--spacing", type=float, default=1.0)
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--workdir", default=None, help="keep the inputs and outputs there (default: a temporary directory)")
    a = ap.parse_args()
    d = a.workdir or tempfile.mkdtemp(prefix="bench_average_")
    os.makedirs(d, exist_ok=True)
    try:
        t0 = time.perf_counter()
        names = make_inputs(d, a.images, a.dims, a.levels, a.seed)
        make_s = time.perf_counter() - t0
        s = repr(a.spacing)
        # transform.sh
        os.makedirs(os.path.join(d, "flow"), exist_ok=True)
        t0 = time.perf_counter()
        run([os.path.join(BIN, "DummyVolumeGenerator"), "bbox.json", s], d)
        for i, v in enumerate(names):
            run([os.path.join(BIN, "VolumeTransform"), v, "dummy.mhd", "-t", f"transforms/{i}.json", "-o", f"flow/transformed{i}.nii.gz"], d)
        run([os.path.join(BIN, "AverageVolumes")] + [f"transformed{i}.nii.gz" for i in range(a.images)], os.path.join(d, "flow"))
        flow_s = time.perf_counter() - t0
        # one process
        t0 = time.perf_counter()
        out = run([os.path.join(BIN, "AverageImage"), "bbox.json", s] + names + ["-o", "one"], d)
        one_s = time.perf_counter() - t0
        phases = {k: float(v) for k, v in re.findall(r"^(read|device|write|total) : ([0-9.]+) s", out, re.M)}
        m = re.search(r"^read : [0-9.]+ s of (\d+) host threads \(device waited ([0-9.]+) s\)", out, re.M)
        setup = re.search(r"^device : [0-9.]+ s \(\+ ([0-9.]+) s set-up\)", out, re.M)
        equal = True
        for name in ("average.nii.gz", "stdev.nii.gz"):
            x, ox, sx = read_volume(os.path.join(d, "flow", name))
            y, oy, sy = read_volume(os.path.join(d, "one", name))
            equal = equal and x.shape == y.shape and np.array_equal(x, y, equal_nan=True) and ox == oy and sx == sy
        grid = re.search(r"grid (\d+) x (\d+) x (\d+)", out)
        voxels = int(grid.group(1)) * int(grid.group(2)) * int(grid.group(3))
        print(json.dumps({
            "images": a.images, "volume_dims": list(a.dims), "grid_dims": [int(g) for g in grid.groups()], "spacing": a.spacing,
            "lattice_levels": a.levels, "outputs_equal": bool(equal),
            "three_tool_flow_s": round(flow_s, 3), "average_image_s": round(one_s, 3),
            "average_image_phases_s": {**phases, "device_setup": float(setup.group(1)) if setup else None,
                                       "device_waited_for_read": float(m.group(2)) if m else None},
            "read_threads": int(m.group(1)) if m else None,
            "device_image_voxels_per_s": round(a.images * voxels / phases["device"], 1) if phases.get("device") else None,
            "inputs_made_s": round(make_s, 3)}))
        if not equal:
            sys.exit(1)
    finally:
        if not a.workdir:
            shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
