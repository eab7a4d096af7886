#!/usr/bin/env python3
"""frog_glm at volume size: the 256^3 grid and the 1 + 7 link chains of scripts/bench_labels.py, 20 images, a
3-column design (intercept, alternating group, centred age), the log Jacobian determinant as the value.

  bench_glm.py [--out FILE]           wall times (host clock around whole calls; every call ends in a synchronisation):
                                      frog_glm_add_jacobian next to frog_chain_sample (determinant only, f32) on the same chain;
                                      frog_glm_finish, the median of 5; frog_glm_permute with 16, 64 and 1000 permutations of the
                                      group column; bin/GroupStats end to end with 100 permutations
  bench_glm.py --trace-run [--depth NZ]   the adds, one finish and one permute of 64, nothing else: the command to run under
                                      `rocprofv3 --kernel-trace --stats -d DIR -o p --output-format csv` or, in a run of its own
                                      on a grid of NZ planes, under `rocprofv3 --pmc ...`
  bench_glm.py --merge DIR            reads DIR's kernel trace, counter files and ab.jsonl (no device needed) and adds the
                                      kernel times, the rates, the counters and the A/B lines
  bench_glm.py --ab LIB               frog_rank_add, frog_chain_sample and frog_chain_reslice through the device library LIB
                                      (a build of another commit, which need not export frog_glm_*): one JSON line"""
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

IMAGES, DISTINCT, P = 20, 4, 3
F64_OPS_PER_S = 3.93e13             # the measured rate of separately rounded f64 operations


def design():
    age = np.array([31, 45, 52, 38, 60, 27, 49, 55, 42, 36, 58, 29, 47, 51, 33, 40, 56, 44, 39, 50], np.float64)
    return np.stack([np.ones(IMAGES), np.arange(IMAGES) % 2, age - age.mean()], axis=1)


def operations(n, p):
    """The f64 operations one thread of the fit kernel executes per voxel and permutation: per image p (p + 1) / 2 additions
    into A (the products come from the table), 2 p for b, 2 p + 3 for its residual; the factor, three solves' worth of
    substitutions for beta and one contrast, and the closing lines."""
    tri = p * (p + 1) // 2
    factor = sum(3 * j + 2 + (p - 1 - j) * (3 * j + 1) for j in range(p))
    solve = p * (p - 1) * 2 + p
    return n * (tri + 4 * p + 3) + factor + 2 * solve + 4 * p + 8


def filled(chains, times=None):
    from frog_amd.volume import GroupGLM
    acc = GroupGLM(GRID, design())
    for i in range(IMAGES):
        ms = timed(lambda: acc.add_jacobian(chains[i % DISTINCT], None, None, True))[1]
        if times is not None and i:
            times.append(ms)
    return acc


def measure(args):
    from frog_amd.chain import Chain, invert
    from frog_amd.volume import glm_draw
    chains = [Chain(invert(chain_links(100 + i))) for i in range(DISTINCT)]
    out = {"what": "scripts/bench_glm.py on one MI355X: %d images (%d distinct chains of 1 matrix + 7 lattices, inverted, in turn) on a 256^3 "
                   "grid at 400/256 mm, value = log Jacobian determinant, a %d-column design, one contrast (the group column); wall times "
                   "are host-clock times of whole calls, copies included" % (IMAGES, DISTINCT, P),
           "voxels": N ** 3, "f64_operations_per_voxel_and_permutation": operations(IMAGES, P), "wall": {}}
    t_sample = [timed(lambda: chains[i % DISTINCT].sample(GRID[1], GRID[2], GRID[0], displacement=False))[1] for i in range(6)][1:]
    t_add = []
    acc = filled(chains, t_add)
    print("adds done", file=sys.stderr, flush=True)
    con = [[0.0, 1.0, 0.0]]
    t_finish = [timed(lambda: acc.finish(con))[1] for _ in range(args.repeats + 1)][1:]
    fit = int((acc.finish(con, fill=-1.0)[1] != -1).sum())
    w = out["wall"]
    w["chain_sample_determinant_f32"], w["glm_add_jacobian"], w["glm_finish"] = stats(t_sample), stats(t_add), stats(t_finish)
    out["fit_voxels"] = fit
    for k in (16, 64, 1000):
        perm, _ = glm_draw(IMAGES, k, 1)
        reps = 1 if k == 1000 else 3
        t = [timed(lambda: acc.permute(con, perm, None, [1]))[1] for _ in range(reps)]
        w[f"glm_permute_{k}"] = dict(stats(t), per_permutation_ms=round(float(np.median(t)) / k, 4))
        print(f"permute {k} done", file=sys.stderr, flush=True)
    acc.close()
    per = w["glm_permute_1000"]["per_permutation_ms"] * 1e-3
    out["permute_f64_operations_per_s_wall"] = round(operations(IMAGES, P) * fit / per, 1)
    out["permute_share_of_f64_rate_wall"] = round(out["permute_f64_operations_per_s_wall"] / F64_OPS_PER_S, 4)
    out["tool"] = tool()
    return out


def tool():
    """bin/GroupStats on the same chains as files, 100 permutations: its phase lines."""
    d = tempfile.mkdtemp(prefix="bench_glm_")
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
        with open(os.path.join(d, "design.csv"), "w") as fh:
            fh.write("intercept,group,age\n" + "\n".join(",".join(repr(float(v)) for v in row) for row in design()) + "\n")
        with open(os.path.join(d, "contrasts.csv"), "w") as fh:
            fh.write("0,1,0\n")
        t0 = time.perf_counter()
        r = subprocess.run([os.path.join(ROOT, "bin", "GroupStats"), "bbox.json", repr(GRID[2][0]), "design.csv", "-c", "contrasts.csv", "-o", "out",
                            "-np", "100"], cwd=d, capture_output=True, text=True, timeout=900)
        wall = time.perf_counter() - t0
        if r.returncode != 0:
            raise RuntimeError(r.stdout[-2000:] + r.stderr[-2000:])
        phases = {k: float(v) for k, v in re.findall(r"^(read|device|write|total) : ([0-9.]+) s", r.stdout, re.M)}
        slabs = re.search(r"stats : (\d+) slab", r.stdout)
        return {"permutations": 100, "wall_s": round(wall, 3), "slabs": int(slabs.group(1)), "phases_s": phases}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def trace_run(args):
    global GRID
    from frog_amd.chain import Chain, invert
    from frog_amd.volume import glm_draw
    GRID = ((N, N, args.depth), GRID[1], GRID[2])
    chains = [Chain(invert(chain_links(100 + i))) for i in range(DISTINCT)]
    chains[0].sample(GRID[1], GRID[2], GRID[0], displacement=False)
    acc = filled(chains)
    acc.finish([[0.0, 1.0, 0.0]])
    acc.permute([[0.0, 1.0, 0.0]], glm_draw(IMAGES, 64, 1)[0], None, [1])
    acc.close()


def merge(directory, out):
    files = glob.glob(os.path.join(directory, "**", "*_kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"one *_kernel_trace.csv expected under {directory}, found {len(files)}")
    kernels = {}
    for r in sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"])):
        name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        if "glm_" in name or "chain_sample" in name:
            kernels.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    out["kernels_under_rocprofv3"] = {k: {"launches": len(t), "median_ms": round(float(np.median(t)), 4), "min_ms": round(min(t), 4),
                                          "max_ms": round(max(t), 4)} for k, t in sorted(kernels.items())}
    fits = [t for k, t in kernels.items() if "glm_fit" in k]
    if fits and len(fits[0]) >= 2:
        # trace_run's launches of the fit kernel: finish (one design), then permute's single launch of 64 permutations
        ms = fits[0][-1] / 64
        ops = out["f64_operations_per_voxel_and_permutation"] * out["fit_voxels"]
        out["permute_kernel"] = {"per_permutation_ms": round(ms, 4), "f64_operations_per_s": round(ops / (ms * 1e-3), 1),
                                 "share_of_f64_rate": round(ops / (ms * 1e-3) / F64_OPS_PER_S, 4),
                                 "values_read_once_bytes": 4 * IMAGES * N ** 3,
                                 "bytes_per_s_over_64_permutations": round(4 * IMAGES * N ** 3 / (fits[0][-1] * 1e-3), 1)}
    counters = {}
    for f in glob.glob(os.path.join(directory, "**", "*_counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "glm_fit" in r["Kernel_Name"]:
                counters.setdefault(r["Counter_Name"], []).append(float(r["Counter_Value"]))
    if counters:
        # per counter the launch with the largest value: permute's launch of 64 permutations (the other is finish's)
        out["permute_kernel_counters_64_permutations"] = {k: max(v) for k, v in sorted(counters.items())}
        depth = os.path.join(directory, "pmc_depth")
        if os.path.exists(depth):
            out["counters_grid_depth"] = int(open(depth).read())
    ab_lines = os.path.join(directory, "ab.jsonl")
    if os.path.exists(ab_lines):
        out["collect_sample_reslice_by_library_in_turn"] = [json.loads(line) for line in open(ab_lines) if line.strip()]
    return out


def ab(args):
    """The collect, sample and reslice calls that existed before frog_glm, through another build of the device library."""
    os.environ["FROG_HIP_LIB"] = os.path.abspath(args.ab)
    from frog_amd import _abi
    _abi.HIP_SYMBOLS = {k: v for k, v in _abi.HIP_SYMBOLS.items() if not k.startswith("frog_glm_")}
    from bench_cover import image_volume
    from frog_amd.chain import Chain, invert
    from frog_amd.volume import RankImages
    chains = [Chain(invert(chain_links(100 + i))) for i in range(2)]
    vol = (image_volume(0), GRID[1], GRID[2])
    acc = RankImages(GRID, 12)
    t_rank = [timed(lambda: acc.add(vol, chains[i % 2], None, 1, 0.0))[1] for i in range(12)][1:]
    acc.close()
    t_sample = [timed(lambda: chains[i % 2].sample(GRID[1], GRID[2], GRID[0], displacement=False))[1] for i in range(8)][1:]
    t_reslice = [timed(lambda: chains[i % 2].reslice(vol[0], vol[1], vol[2], GRID[0], GRID[1], GRID[2]))[1] for i in range(8)][1:]
    print(json.dumps({"library": args.ab, "rank_add": stats(t_rank), "chain_sample": stats(t_sample), "chain_reslice": stats(t_reslice)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_glm.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--depth", type=int, default=N)
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
