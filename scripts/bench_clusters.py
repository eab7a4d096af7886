#!/usr/bin/env python3
"""The cluster-extent test at volume size: scripts/bench_glm.py's case -- the 256^3 grid, 20 images, a 3-column
design, the log Jacobian determinant as the value -- with a thousand permutations of the group column, the cluster-forming
threshold 3.0 and connectivity 26.

  bench_clusters.py [--out FILE]   wall times (host clock around whole calls; every call ends in a synchronisation):
                                   frog_glm_permute and frog_glm_permute_clusters with the thousand permutations,
                                   frog_clusters_finish over the thousand slots, one frog_clusters_labels; the set voxels and the
                                   largest extents of the slots; bin/GroupStats end to end with 100 permutations, with and
                                   without -ct
  bench_clusters.py --ab LIB       frog_glm_permute (64 permutations, the median of 9 calls) through the device library LIB
                                   (a build of another commit, which need not export frog_clusters_*): one JSON line
  bench_clusters.py --merge FILE   adds FILE's --ab lines (no device needed) to the output file"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_glm import IMAGES, DISTINCT, filled              # noqa: E402
from bench_labels import GRID, N, chain_links, stats, timed  # noqa: E402

PERMS, THRESHOLD, CONNECTIVITY = 1000, 3.0, 26
CONTRAST = [[0.0, 1.0, 0.0]]
NEW_SYMBOLS = ("frog_components", "frog_clusters_", "frog_glm_permute_clusters")


def measure(args):
    from frog_amd.chain import Chain, invert
    from frog_amd.volume import ClusterSink, glm_draw
    chains = [Chain(invert(chain_links(100 + i))) for i in range(DISTINCT)]
    acc = filled(chains)
    perm, _ = glm_draw(IMAGES, PERMS, 1)
    out = {"what": "scripts/bench_clusters.py on one MI355X: scripts/bench_glm.py's group (%d images, 256^3 grid, 3 columns, one contrast), %d "
                   "permutations of the group column, threshold %.1f, connectivity %d, one-sided; wall times are host-clock times of whole "
                   "calls, copies included" % (IMAGES, PERMS, THRESHOLD, CONNECTIVITY),
           "voxels": N ** 3, "permutations": PERMS, "wall": {}}
    w = out["wall"]
    acc.permute(CONTRAST, perm[:64], None, [1])              # the first launches of a process
    plain = [timed(lambda: acc.permute(CONTRAST, perm, None, [1])) for _ in range(args.repeats)]
    w["glm_permute_1000"] = dict(stats([t for _, t in plain]), per_permutation_ms=round(float(np.median([t for _, t in plain])) / PERMS, 4))
    t_fill, t_finish, t_create = [], [], []
    for r in range(args.repeats):
        sink, ms = timed(lambda: ClusterSink(GRID, PERMS, 1, THRESHOLD, False, CONNECTIVITY))
        t_create.append(ms)
        got, ms = timed(lambda: acc.permute_clusters(sink, CONTRAST, perm, None, [1]))
        t_fill.append(ms)
        assert got[0].tobytes() == plain[0][0][0].tobytes() and got[1].tobytes() == plain[0][0][1].tobytes()
        extents, ms = timed(sink.finish)
        t_finish.append(ms)
        again, ms = timed(sink.finish)
        t_finish.append(ms)
        assert (again == extents).all()
        if r + 1 < args.repeats:
            sink.close()
    w["clusters_create"] = stats(t_create)
    w["glm_permute_clusters_1000"] = dict(stats(t_fill), per_permutation_ms=round(float(np.median(t_fill)) / PERMS, 4))
    w["clusters_finish_1000_slots"] = dict(stats(t_finish), per_slot_ms=round(float(np.median(t_finish)) / PERMS, 4))
    (labels, found), ms = timed(lambda: sink.labels(0, 0))
    w["clusters_labels_one_slot"] = {"ms": round(ms, 3), "components": found}
    set_voxels = [int(sink.mask(k, 0).sum()) for k in (0, 1, 2, 3, 500, 999)]
    out["set_voxels_of_slots_0_1_2_3_500_999"] = set_voxels
    out["largest_extent"] = {"observed": int(extents[0, 0, 0]), "null_median": float(np.median(extents[1:, 0, 0])), "null_max": int(extents[1:, 0, 0].max())}
    out["masks_per_launch"] = min(PERMS, 64)
    out["device_bytes"] = {"masks": PERMS * ((N ** 3 + 31) // 32) * 4, "workspace_per_mask_of_a_launch": 8 * N ** 3}
    sink.close()
    acc.close()
    out["noise"] = noise(args, perm)
    out["tool"] = {"without_ct": tool(False), "with_ct": tool(True)}
    return out


def noise(args, perm):
    """The same design on 20 volumes of white N(0, 1) noise: what the masks of a null look like, which the group above, four
    distinct chains in turn, does not show (most of its permutations leave no voxel beyond the threshold, two leave millions)."""
    from bench_glm import design
    from frog_amd.volume import ClusterSink, GroupGLM
    rng = np.random.default_rng(24)
    acc = GroupGLM(GRID, design())
    for _ in range(IMAGES):
        acc.add(rng.standard_normal((N, N, N), np.float32))
    out = {"what": "%d volumes of white N(0, 1) noise on the grid, the same design, permutations, threshold and connectivity" % IMAGES}
    plain = [timed(lambda: acc.permute(CONTRAST, perm, None, [1]))[1] for _ in range(args.repeats)]
    out["glm_permute_1000"] = dict(stats(plain), per_permutation_ms=round(float(np.median(plain)) / PERMS, 4))
    t_fill, t_finish = [], []
    for r in range(args.repeats):
        sink = ClusterSink(GRID, PERMS, 1, THRESHOLD, False, CONNECTIVITY)
        t_fill.append(timed(lambda: acc.permute_clusters(sink, CONTRAST, perm, None, [1]))[1])
        extents, ms = timed(sink.finish)
        t_finish.append(ms)
        if r + 1 < args.repeats:
            sink.close()
    out["glm_permute_clusters_1000"] = dict(stats(t_fill), per_permutation_ms=round(float(np.median(t_fill)) / PERMS, 4))
    out["clusters_finish_1000_slots"] = dict(stats(t_finish), per_slot_ms=round(float(np.median(t_finish)) / PERMS, 4))
    (labels, found), ms = timed(lambda: sink.labels(1, 0))
    out["clusters_labels_slot_1"] = {"ms": round(ms, 3), "components": found}
    out["set_voxels_of_slots_0_1_2_3_500_999"] = [int(sink.mask(k, 0).sum()) for k in (0, 1, 2, 3, 500, 999)]
    out["largest_extent"] = {"observed": int(extents[0, 0, 0]), "null_median": float(np.median(extents[1:, 0, 0])), "null_max": int(extents[1:, 0, 0].max())}
    sink.close()
    acc.close()
    return out


def tool(clusters, extra=()):
    """bin/GroupStats on bench_glm's files with 100 permutations (and the options `extra`): its phase lines."""
    import re
    import shutil
    import tempfile
    from bench_glm import design
    d = tempfile.mkdtemp(prefix="bench_clusters_")
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
                            "-np", "100"] + (["-ct", repr(THRESHOLD), "-cc", str(CONNECTIVITY)] if clusters else []) + list(extra),
                           cwd=d, capture_output=True, text=True, timeout=900)
        wall = time.perf_counter() - t0
        if r.returncode != 0:
            raise RuntimeError(r.stdout[-2000:] + r.stderr[-2000:])
        phases = {k: float(v) for k, v in re.findall(r"^(read|device|write|total) : ([0-9.]+) s", r.stdout, re.M)}
        return {"permutations": 100, "wall_s": round(wall, 3), "phases_s": phases}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def ab(args):
    """frog_glm_permute, which existed before frog_clusters, through another build of the device library."""
    os.environ["FROG_HIP_LIB"] = os.path.abspath(args.ab)
    from frog_amd import _abi
    _abi.HIP_SYMBOLS = {k: v for k, v in _abi.HIP_SYMBOLS.items() if not k.startswith(NEW_SYMBOLS)}
    from frog_amd.chain import Chain, invert
    from frog_amd.volume import glm_draw
    chains = [Chain(invert(chain_links(100 + i))) for i in range(DISTINCT)]
    acc = filled(chains)
    perm, _ = glm_draw(IMAGES, 64, 1)
    t = [timed(lambda: acc.permute(CONTRAST, perm, None, [1]))[1] for _ in range(10)][1:]
    acc.close()
    print(json.dumps({"library": args.ab, "glm_permute_64": stats(t)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_clusters.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ab")
    ap.add_argument("--merge")
    args = ap.parse_args()
    if args.ab:
        return ab(args)
    if args.merge:
        out = json.load(open(args.out))
        out["glm_permute_by_library_in_turn"] = [json.loads(line) for line in open(args.merge) if line.strip().startswith("{")]
    else:
        out = measure(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
