"""Child process of tests/test_gpu_scatter_mfma.py: the designed scatter cases through whichever device library FROG_HIP_LIB
names, results into an .npz (the library is chosen once per process, so the two builds need two processes).
usage: run_scatter_cases.py OUT.npz"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from frog_amd.image_group import ImageGroup     # noqa: E402
import scatter_cases as sc                     # noqa: E402

out = {}
for name, (group, brick, box) in sc.CASES.items():
    os.environ["FROG_BRICK"] = str(brick)       # read when the context is created
    pairs = sc.pairs(group)
    g = ImageGroup(pairs, **sc.OPTIONS)
    g.setupLinearTransforms(); g.transformPoints(); g.transformPoints(True)
    info = g.setupDeformableTransforms(0) if box is None else g.deformable_setup_bounds(0, *box)
    g.transformPoints(); g.updateStats()
    out[f"{name}/dims"] = np.array(list(info.dims))
    k = g.num_grids() - 1
    for step in range(sc.STEPS):
        out[f"{name}/E{step}"] = np.array(g.updateDeformableTransforms(sc.ALPHA))
        out[f"{name}/lattice{step}"] = np.stack([g.grid(i, k)[1] for i in range(pairs.n_images)])
        if step == 0:
            out[f"{name}/sums"] = g.point_sums()
        g.transformPoints()
        out[f"{name}/xyz2_{step}"] = g.points()[1]
    out[f"{name}/strays"] = np.array(g.stray_points())
    g.close()
np.savez(sys.argv[1], **out)
