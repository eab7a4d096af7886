"""The designed group of tests/lattice_design.py on the CPU: the point classes are there, the frame keeps the group exact, and
the oracle -- the reference's arithmetic -- stays inside the derived bound of the f64 restatement at every (image, node,
component), with the transform equal to the restatement's to the last bit.  The same checks run on the device in
tests/test_gpu_lattice_design.py."""
import numpy as np
import pytest

from frog_amd import _abi
from oracle.oracle_api import OracleGroup
import lattice_design as ld

ALPHA = 1.0


@pytest.fixture(scope="module")
def group():
    po, xyz, blocks = ld.build()
    return ld.pairs(), po, xyz, blocks


def oracle_at(pairs, level):
    ref = OracleGroup(pairs.model, _abi.FrogOptions.default(**ld.OPTIONS))
    ref.setup_stats()
    ref.linear_init(); ref.transform_points(); ref.transform_points(True)
    info = ref.deformable_setup(level, _abi.FrogGridInfo())
    ref.transform_points(); ref.update_stats()
    return ref, info


def test_the_designed_classes_are_there(group):
    pairs, po, xyz, blocks = group
    img0 = xyz[po[0]:po[1]]
    for i in range(ld.N_IMAGES):                             # the frame, and nothing outside it
        a = xyz[po[i]:po[i + 1]]
        assert np.array_equal(a[0], [0, 0, 0]) and np.array_equal(a[1], [64, 64, 64]) and a.min() >= 0 and a.max() <= 64
    assert po[4] - po[3] == 2 and po[5] - po[4] == 3 and np.array_equal(xyz[po[4] + 2], [32, 32, 32])
    for i in (1, 2):                                        # moved by at most 0.02 per axis
        assert np.abs(xyz[po[i]:po[i + 1]].astype(np.float64) - img0).max() <= 0.02
    c = ld.classes(img0, ld.Lattice.level(0), brick=4)
    assert min(c["fraction_zero"]) >= 256, c
    assert min(c["cell_differs"]) >= 64 and c["brick_face"] >= 16, c
    assert c["tails_two_axes"] >= 25 and c["tails_three_axes"] >= 25 and c["lone_tails"] >= 1, c
    assert c["largest_cell"] > 1000 > ld.SCATTER_CHUNK, c
    assert c["bricks"] == ld.FULL_BRICKS, c
    # the faces hold 0, 64 and the brick faces of both brick edges and of level 1 (multiples of 16; 48 is one at level 0 for both)
    for v in (0.0, 16.0, 32.0, 48.0, 64.0):
        assert np.count_nonzero(np.any(img0 == np.float32(v), axis=1)) >= 100, v
    for level, brick in ((0, 8), (1, 4), (1, 8), (3, 4)):   # the other lattices and brick edges the device tests run
        c = ld.classes(img0, ld.Lattice.level(level), brick)
        assert min(c["fraction_zero"]) >= 256 and min(c["cell_differs"]) >= 64 and c["brick_face"] >= 16, (level, brick, c)


def test_the_frame_keeps_the_group_exact(group):
    pairs, po, xyz, blocks = group
    for level in (0, 1, 3):
        ref, info = oracle_at(pairs, level)
        assert np.array_equal(ref.xyz(), xyz) and np.array_equal(ref.xyz2(), xyz)
        for i in range(ld.N_IMAGES):
            assert np.array_equal(ref.matrix(i), np.eye(4)), i
        cells, spacing, origin, dims = ld.LATTICES[level]
        assert list(info.dims) == [dims] * 3 and list(info.origin) == [origin] * 3 and list(info.spacing) == [spacing] * 3


@pytest.mark.parametrize("level", [0, 1, 3])
def test_the_oracle_stays_inside_the_bound(group, level):
    """Two steps (the second from non-zero coefficients).  Measured: the worst err / bound of the oracle is recorded in
    DESIGN.md section 2a."""
    pairs, po, xyz, blocks = group
    ref, info = oracle_at(pairs, level)
    lat = ld.Lattice.of(info)
    worst = 0.0
    for it in range(2):
        c_prev = [ref.grid(i, 0, _abi.FrogGridInfo())[1] for i in range(ld.N_IMAGES)]
        x2 = ref.xyz2()
        want_e, longest = ld.energy(po, blocks, x2)
        assert longest < 0.095                               # every weight is the constant 1
        e = ref.deformable_step(ALPHA)
        sums = ref.point_sums()
        assert set(np.unique(sums[:, 3])) == {0.0, 2.0}
        assert abs(e - want_e) <= 1e-6 * want_e
        r = ld.step(lat, po, ref.xyz(), sums, c_prev, ALPHA, touched_only=level == 3)
        gw = r["gw"]
        assert np.all((gw == 0) | (gw >= 2.0 ** -140))       # no decision hangs on underflow
        if level < 3:
            assert np.any((gw > 0) & (gw < 2.0 ** -126))     # ... and a node lives on a denormal weight alone
        for i in range(ld.N_IMAGES):
            c = ref.grid(i, 0, _abi.FrogGridInfo())[1]
            ratio, at = ld.worst_ratio(r["new"][i], r["bound"][i], c[r["nodes"]])
            assert ratio <= 2.0, (level, it, i, ratio, at)
            worst = max(worst, ratio)
            if level == 3:                                   # nodes nothing reaches: the previous coefficients' mean removed
                rest = np.ones(lat.n_cp, bool); rest[r["nodes"]] = False
                assert not np.any(c[rest])                   # (the scatter bins Point::xyz, which does not move)
        ref.transform_points()
        got = ref.xyz2()
        for i in range(ld.N_IMAGES):
            c = ref.grid(i, 0, _abi.FrogGridInfo())[1]
            want, _ = ld.transform(lat, xyz[po[i]:po[i + 1]], c)
            assert np.array_equal(got[po[i]:po[i + 1]], want), (level, it, i)
    disp = np.abs(ref.xyz2().astype(np.float64) - xyz).max()
    assert disp >= 2.0 ** 10 * 2.0 ** -17                    # 2^10 ulps of 64: the steps moved the points
    print(f"level {level}: worst err / bound of the oracle {worst:.3f}, max |disp| {disp:.4f}")
