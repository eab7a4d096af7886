#!/usr/bin/env python3
"""cfg 3 (100 images x 20 000 keypoints, 1e8 half-links) over the reference's FULL default schedule (-li 50 -dl 3 -di 200,
regrids as the diffeomorphism guard asks for them), HIP path and oracle free-running from the same pairs: the parity numbers
of tests/test_gpu_round3.py::test_config3_free_running_schedule_against_the_oracle (which runs 10 + 3 x 10 iterations) for a
whole registration.  Takes ~6 minutes of oracle time on the GPU box; writes a JSON summary.

    python3 scripts/parity_full_schedule.py [out.json] [linear] [per_level]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np                                               # noqa: E402

from frog_amd import _abi, schedule                              # noqa: E402
from frog_amd.image_group import ImageGroup                      # noqa: E402
from frog_amd.pairs import Pairs                                 # noqa: E402
from oracle.oracle_api import OracleGroup                        # noqa: E402
from lattice_util import lattice_deviation, node_weights        # noqa: E402
from gpu_util import relerr                                      # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else "gpurun_out/parity_full_schedule.json"
    li = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    di = int(sys.argv[3]) if len(sys.argv) > 3 else 200
    dl = 3
    t0 = time.time()
    pairs = Pairs.synthetic(100, 20000, 10101, seed=1)
    g = ImageGroup(pairs)
    ref = OracleGroup(pairs.model, _abi.FrogOptions.default())
    ref.setup_stats()
    po = np.asarray(pairs.point_offset)
    e_dev, e_ref, snapshots, levels, count = [], [], [], [], {"rejects": 0, "matrices": 0.0}

    def on(tag, sides, e=None, infos=None):
        kind = schedule.kind(tag)
        if kind in ("linear", "deformable"):
            e_dev.append(e[0]); e_ref.append(e[1])
            it = tag[-1] + 1
            if kind == "linear" and it % 10 == 0:
                print(f"[{time.time() - t0:6.0f}s] linear {it}/{li}  E {e[0]:.6f} / {e[1]:.6f}", flush=True)
            if kind == "deformable" and it % 25 == 0:
                print(f"[{time.time() - t0:6.0f}s] level {tag[1]} iteration {it}/{di}  lattices so far {len(levels)}  E {e[0]:.6f} / {e[1]:.6f}", flush=True)
        elif kind == "linear_done":
            for i in range(pairs.n_images):
                m, mr = g.matrix(i), ref.matrix(i)
                count["matrices"] = max(count["matrices"], relerr(np.diag(m)[:3], np.diag(mr)[:3]), relerr(m[:3, 3], mr[:3, 3]))
        elif kind == "setup":
            assert list(infos[0].dims) == list(infos[1].dims), f"lattice dimensions differ at level {tag[1]}"
            snapshots.append(ref.xyz().copy()); levels.append(tag[1])
        elif kind == "step" and e[0] < 0:
            count["rejects"] += 1
    grids = schedule.run([g, ref], li, [di] * dl, on=on)
    rejects, worst_m = count["rejects"], count["matrices"]
    e_dev, e_ref = np.array(e_dev), np.array(e_ref)
    res = {"workload": f"100 images x 20000 keypoints, {pairs.n_half_links} half-links, -li {li} -dl {dl} -di {di}",
           "iterations": int(len(e_dev)), "guard_rejections": rejects, "grids_per_level": grids,
           "E_max_rel_dev": float(np.max(np.abs(e_dev - e_ref) / e_ref)), "E_final": [float(e_dev[-1]), float(e_ref[-1])],
           "matrices_max_rel_dev": worst_m, "lattices": []}
    for k in range(ref.num_grids()):
        w = node_weights(ref, k, po, snapshots[k])
        worst = {"lattice": k, "level": levels[k], "raw": 0.0, "weighted": 0.0, "field": 0.0}
        for i in range(pairs.n_images):
            d = lattice_deviation(g, ref, k, i, snapshots[k][po[i]:po[i + 1]], w)
            for key in ("raw", "weighted", "field"):
                worst[key] = max(worst[key], d[key])
            worst["weak_nodes"], worst["nodes"] = d["weak"], d["nodes"]
        res["lattices"].append(worst)
        print(f"[{time.time() - t0:6.0f}s] lattice {k}: {worst}", flush=True)
    res["final_xyz_rel_dev"] = relerr(g.points()[0], ref.xyz())
    res["seconds"] = time.time() - t0
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
