"""BASELINE.json configs[4] at full size on ONE GPU: 500 images x 20 000 keypoints, ~60 partner images each,
~2.5e8 pairs (5e8 half-links), five deformable levels, -gd 1.  (The configuration is quoted for 8 GPUs; it fits one
MI355X's 288 GB, which is what makes this test possible on the one-GPU box.)

Against the oracle: one linear step of a sub-range of images from identical inputs (the oracle walks 4 of the 500
images in seconds).  Without it, properties that do not depend on size: the lattices of a level sum to zero over the
images (imageGroup.cxx:417-423), the census adds up, the energy is finite and falls, the diffeomorphism guard rejects
an oversize step without touching the state, the culling list leaves the false matches out."""
import numpy as np
import pytest

from frog_amd import _abi, schedule
from frog_amd.image_group import ImageGroup
from frog_amd.pairs import Pairs
from oracle.oracle_api import OracleGroup
from gpu_util import relerr

pytestmark = pytest.mark.gpu


def test_config5_on_one_gpu():
    pairs = Pairs.synthetic(500, 20000, 16667, seed=1, partners_per_image=60)
    assert 2.2e8 < pairs.n_pairs < 2.8e8
    g = ImageGroup(pairs)
    g.setupLinearTransforms(); g.transformPoints()
    E = []
    for it in range(4):
        if it % 10 == 0:
            g.updateStats()
        E.append(g.updateLinearTransforms()); g.transformPoints()
    assert all(np.isfinite(E)) and E[-1] < E[0]

    # ---- one oracle step on images [0, 4) from identical coordinates and mixtures
    ref = OracleGroup(pairs.model, _abi.FrogOptions.default())
    ref.setup_stats(); ref.linear_init()
    ref.set_xyz2(g.points()[1])
    for i in range(pairs.n_images):
        ref.set_em(i, g.em(i))
    for i in range(4):                       # the oracle's matrices of the sub-range = the device's current ones
        ref.L.frogo_set_matrix(ref.h, i, g.matrix(i).ravel().ctypes.data_as(_abi.c_double_p))
    ref.set_range(0, 4)
    ref.linear_step_local()
    g.updateLinearTransforms()
    for i in range(4):
        assert relerr(g.matrix(i)[:3, :], ref.matrix(i)[:3, :]) < 1e-6, f"image {i}"
    del ref
    g.transformPoints()

    # ---- five levels, a few steps each
    g.transformPoints(True)
    c0 = g.countInliers()
    assert sum(c.pairs for c in c0) == pairs.n_half_links
    state, e_level = {}, []           # the current lattice's info, the level's accepted energies

    def on(tag, sides, e=None, infos=None):
        kind = schedule.kind(tag)
        if kind == "setup":
            state["info"] = infos[0]
        elif kind == "deformable":
            e_level.append(e[0])
        elif kind == "level_done":
            level, info = tag[1], state["info"]
            assert all(np.isfinite(e_level)) and e_level[-1] <= e_level[0]
            if level <= 1:
                # zero cross-image mean, all 500 images (small lattices only: the finest is 12 MB per image)
                k = g.num_grids() - 1
                tot, mx = None, 0.0
                for i in range(pairs.n_images):
                    c = g.grid(i, k)[1].astype(np.float64)
                    tot = c if tot is None else tot + c
                    mx = max(mx, float(np.max(np.abs(c))))
                assert np.max(np.abs(tot)) <= 1e-5 * max(mx, 1e-3) * pairs.n_images
            if level == 4:
                n_cp = info.dims[0] * info.dims[1] * info.dims[2]
                assert n_cp > 2e5                                        # the HBM-bound stress: a lattice of ~1e6 control points per image
                # the guard: an absurd step is rejected and leaves the state alone (imageGroup.cxx:434-439)
                before = g.grid(7, g.num_grids() - 1)[1].copy()
                x_before = g.points()[1][:1000].copy()
                assert g.updateDeformableTransforms(1e4) == -1.0
                g.transformPoints()
                assert np.array_equal(g.grid(7, g.num_grids() - 1)[1], before)
                assert np.array_equal(g.points()[1][:1000], x_before)
    for level in range(5):
        e_level.clear()
        schedule.run_level([g], level, 3, 10, 0.02, on)
    c1 = g.countInliers()
    assert sum(c.pairs for c in c1) == pairs.n_half_links
    # every point was scattered through the LDS tile of the brick it was sorted into (round 2 found a launch past 2^32
    # threads in the cell-order pass of this very configuration: 60 % of the points went through global atomics)
    assert g.stray_points() == 0
    built, listed, owned = g.cull_stats()
    assert built >= 1 and owned == pairs.n_half_links and 0 < listed < 0.9 * owned


def test_config5_group_sharded_eight_ways_on_one_gpu(tmp_path):
    """configs[4] is quoted for 8 GPUs: its group (4.6e8 half-links) through `bin/frog -ngl 8` -- eight contexts with shards of
    62-63 images on the one GPU, every collective host-staged -- against the one-context run (scripts/cfg5_sharded_rehearsal.py:
    levels 0-2, since the files of levels 3-4 of 500 images are tens of GB): energies, matrices and lattices equal, census
    equal, the eight replicas bit-equal."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "cfg5_sharded.json"
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "cfg5_sharded_rehearsal.py"), str(out)], capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.load(open(out))
    assert res["contexts"] == 8 and res["replicas_identical"] and res["iterations"] == 12
    assert res["E_max_rel_dev"] < 1e-5 and res["matrices_max_rel_dev"] < 1e-6 and res["lattices_max_rel_dev"] < 1e-5
    assert res["half_pairs"][0] == res["half_pairs"][1] > 4e8
