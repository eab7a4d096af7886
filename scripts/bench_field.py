#!/usr/bin/env python3
"""frog_chain_sample and the field link at volume size: the 1 + 7 link chain and the 256^3 grid of
scripts/bench_chain.py, the 256^3 int16 reslice of scripts/bench_register_and_reslice.py.

  bench_field.py [--out FILE] [--baseline-lib LIB]   wall times (host clock around calls that end in a device-to-host copy),
                                                     median and minimum of --repeats; with --baseline-lib the check and
                                                     the reslice are also timed in a child process on that build of
                                                     libfrog_hip.so (FROG_HIP_LIB), alternating with this one
  bench_field.py --trace-run                         the same calls, twice each, and nothing else: the command to run under
                                                     `rocprofv3 --kernel-trace --stats -d DIR -o p --output-format csv`
  bench_field.py --merge DIR [--out FILE]            reads DIR's kernel trace (no device needed) and adds the kernel times
scripts/profile_field.sh runs the three in that order and leaves profiles/field_sample.json."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRID = ((0.0, 0.0, 0.0), (400 / 256,) * 3, (256, 256, 256))
# the kernels of one pass of calls(), in launch order
PASS = ["check", "sample_determinant", "sample_displacement_forward", "sample_displacement_inverse", "reslice_inverse_chain",
        "reslice_field_link"]
KERNELS = ["chain_check_kernel", "chain_sample_kernel", "chain_sample_kernel", "chain_sample_kernel", "reslice_kernel", "reslice_kernel"]


def chain_links(amplitude):
    from frog_amd.chain import Link
    rng = np.random.default_rng(1)
    M = np.eye(4); M[:3, 3] = [3, -2, 1]
    links = [Link.linear(M)]
    for n in (4, 4, 8, 8, 16, 16, 16):
        dims = (n + 3, n + 3, n + 3)
        sp = tuple(400.0 / n for _ in range(3))
        links.append(Link.bspline(dims, tuple(-s for s in sp), sp, (amplitude * rng.normal(size=(dims[0] ** 3, 3))).astype(np.float32)))
    return links


def volume():
    z, y, x = np.meshgrid(np.arange(256), np.arange(256), np.arange(256), indexing="ij")
    return (1000 + 500 * np.sin(x / 9.0) * np.cos(y / 11.0) + 2 * z).astype(np.int16)


def timed(fn, repeats):
    fn()                                                                # warm-up: code object load, first allocations
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter(); out = fn(); t.append((time.perf_counter() - t0) * 1e3)
    return out, {"median_ms": round(float(np.median(t)), 3), "min_ms": round(min(t), 3), "repeats": repeats}


def baseline_child(repeats):
    """check and reslice only, on whatever FROG_HIP_LIB names (a build without frog_chain_sample loads too)."""
    from frog_amd import _abi
    _abi.HIP_SYMBOLS.pop("frog_chain_sample", None)                    # not called here; an older build does not export it
    from frog_amd.chain import Chain, invert
    check_chain, inverse = Chain(chain_links(2.0)), Chain(invert(chain_links(1.0)))
    vol, (o, s, d) = volume(), GRID
    _, t_check = timed(lambda: check_chain.check(*GRID), repeats)
    _, t_reslice = timed(lambda: inverse.reslice(vol, o, s, d, o, s, 1, 0.0), repeats)
    print(json.dumps({"check": t_check, "reslice_inverse_chain": t_reslice}))


def measure(args):
    from frog_amd.chain import Chain, Link, invert
    o, s, d = GRID
    forward = chain_links(2.0)                                          # bench_chain.py's chain (it folds: amplitude 2)
    smooth = chain_links(1.0)                                           # bench_register_and_reslice.py's chain
    c_fwd, c_inv = Chain(forward), Chain(invert(smooth))
    vol = volume()
    out = {"what": "scripts/bench_field.py on one MI355X: 1 matrix + 7 lattices (4, 4, 8, 8, 16, 16, 16 cells over 400 mm), "
                   "256^3 nodes at 400/256 mm; wall times are host-clock times of whole calls, copies to the host included",
           "nodes": 256 ** 3, "wall": {}}
    w = out["wall"]
    (n_neg, min_det), w["check"] = timed(lambda: c_fwd.check(*GRID), args.repeats)
    (_, det), w["sample_determinant_f32"] = timed(lambda: c_fwd.sample(*GRID, displacement=False), args.repeats)
    _, w["sample_displacement_forward_f32"] = timed(lambda: c_fwd.sample(*GRID, determinant=False), args.repeats)
    (inv_disp, _), w["sample_displacement_inverse_f32"] = timed(lambda: c_inv.sample(*GRID, determinant=False), args.repeats)
    _, w["sample_both_forward_f64"] = timed(lambda: c_fwd.sample(*GRID, dtype=np.float64), max(2, args.repeats // 2))
    assert int((det < 0).sum()) == n_neg and det.min() == np.float32(min_det)
    out["check_result"] = {"negative": n_neg, "min_determinant": min_det}
    w["sample_determinant_over_check"] = round(w["sample_determinant_f32"]["median_ms"] / w["check"]["median_ms"], 3)
    # the collapse: the Newton inverse of the 1 + 7 links per voxel, against one field link made from it on the output grid
    ref, w["reslice_inverse_chain"] = timed(lambda: c_inv.reslice(vol, o, s, d, o, s, 1, 0.0), args.repeats)
    c_field = Chain([Link.field(d, o, s, inv_disp)])
    got, w["reslice_field_link"] = timed(lambda: c_field.reslice(vol, o, s, d, o, s, 1, 0.0), args.repeats)
    diff = np.abs(got.astype(np.int32) - ref.astype(np.int32))
    out["collapse"] = {"voxels_that_differ_percent": round(float((diff > 0).mean() * 100), 5), "largest_difference_grey_levels": int(diff.max()),
                       "speedup": round(w["reslice_inverse_chain"]["median_ms"] / w["reslice_field_link"]["median_ms"], 2),
                       "sampling_ms": w["sample_displacement_inverse_f32"]["median_ms"]}
    if args.baseline_lib:
        # the same two calls on another build of the device library, this build and that one in turn
        rounds = {"baseline": [], "this": []}
        for _ in range(2):
            for name, lib in (("baseline", os.path.abspath(args.baseline_lib)), ("this", "libfrog_hip.so")):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--baseline-child", "--repeats", str(args.repeats)],
                                   env=dict(os.environ, FROG_HIP_LIB=lib), capture_output=True, text=True, timeout=300)
                if r.returncode != 0:
                    raise RuntimeError(r.stdout[-2000:] + r.stderr[-2000:])
                rounds[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
        out["against_baseline_library"] = rounds
    return out


def trace_run():
    from frog_amd.chain import Chain, Link, invert
    o, s, d = GRID
    c_fwd, c_inv = Chain(chain_links(2.0)), Chain(invert(chain_links(1.0)))
    vol = volume()
    for _ in range(2):
        c_fwd.check(*GRID)
        c_fwd.sample(*GRID, displacement=False)
        c_fwd.sample(*GRID, determinant=False)
        inv_disp, _ = c_inv.sample(*GRID, determinant=False)
        c_inv.reslice(vol, o, s, d, o, s, 1, 0.0)
        Chain([Link.field(d, o, s, inv_disp)]).reslice(vol, o, s, d, o, s, 1, 0.0)


def merge(directory, out):
    """Kernel times of the second pass of trace_run() from rocprofv3's kernel trace (rows in start order)."""
    files = glob.glob(os.path.join(directory, "**", "*_kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"one *_kernel_trace.csv expected under {directory}, found {len(files)}")
    rows = []
    for r in csv.DictReader(open(files[0])):
        name = r["Kernel_Name"]
        if any(k in name for k in set(KERNELS)):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name))
    rows.sort()
    if len(rows) != 2 * len(PASS):
        raise SystemExit(f"{2 * len(PASS)} chain kernels expected in the trace, found {len(rows)}")
    kernels = {}
    for label, want, (t0, t1, name) in zip(PASS, KERNELS, rows[len(PASS):]):
        if want not in name:
            raise SystemExit(f"{label}: {want} expected, the trace has {name}")
        kernels[label] = {"kernel": name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0], "ms": round((t1 - t0) / 1e6, 3)}
    out["kernels_under_rocprofv3"] = kernels
    out["kernel_sample_determinant_over_check"] = round(kernels["sample_determinant"]["ms"] / kernels["check"]["ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_sample.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--baseline-lib")
    ap.add_argument("--baseline-child", action="store_true")
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--merge")
    args = ap.parse_args()
    if args.baseline_child:
        return baseline_child(args.repeats)
    if args.trace_run:
        return trace_run()
    out = merge(args.merge, json.load(open(args.out))) if args.merge else measure(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
