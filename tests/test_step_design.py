"""The many-image group of tests/step_design.py on the CPU: the group is what its docstring says, the oracle -- the reference's
arithmetic -- stays inside the restatement's derived bound at every (image, node, component) for image counts on both sides of
a pass of 64 and with a fixed image (no mean, lattice_design.step(mean_over=None)), and the oracle's guard decides by the strict
`>` at a limit placed on an attained coefficient.  The same checks run on the device in tests/test_gpu_step_design.py."""
import numpy as np
import pytest

from frog_amd import _abi
from oracle.oracle_api import OracleGroup
import lattice_design as ld
import step_design as sd

ALPHA = 1.0


def oracle_at(n_images, **opt):
    pairs = sd.pairs(n_images)
    ref = OracleGroup(pairs.model, _abi.FrogOptions.default(**{**sd.OPTIONS, **opt}))
    ref.setup_stats()
    ref.linear_init(); ref.transform_points(); ref.transform_points(True)
    info = ref.deformable_setup(0, _abi.FrogGridInfo())
    ref.transform_points(); ref.update_stats()
    return ref, info


def coefficients(ref, n_images):
    return np.stack([ref.grid(i, 0, _abi.FrogGridInfo())[1] for i in range(n_images)])


@pytest.mark.parametrize("n_images", [2, 3, 65, 513])
def test_the_group_is_as_designed(n_images):
    po, xyz, blocks = sd.build(n_images)
    for i in range(n_images):                                   # the frame, and nothing outside it
        a = xyz[po[i]:po[i + 1]]
        assert np.array_equal(a[0], [0, 0, 0]) and np.array_equal(a[1], [64, 64, 64]) and a.min() >= 0 and a.max() <= 64
        assert len(a) == sd.layout(i, n_images)[1]
        if i >= 2:
            assert len(a) <= 2 + sd.BASE
    # image i is a copy of the base set moved by at most 0.02 per axis: against image 0, part by part
    l0, _ = sd.layout(0, n_images)
    for i in range(1, n_images):
        li, _ = sd.layout(i, n_images)
        for name, n in (("shared", sd.N_SHARED), ("thirds", sd.N_THIRDS), ("last", sd.N_LAST), ("arms", sum(sd.ARMS.values()))):
            if li[name] is not None and l0[name] is not None:
                d = xyz[po[i] + li[name]:po[i] + li[name] + n].astype(np.float64) - xyz[po[0] + l0[name]:po[0] + l0[name] + n]
                assert np.abs(d).max() <= 0.02, (i, name)
    assert sd.link_lengths(po, blocks, xyz).max() < 0.095       # every weight is the constant 1
    assert all(i < j for i, j, p, q in blocks) and all(j - i in (1, 3) for i, j, p, q in blocks)
    n_links = sd.links_per_point(po, blocks)
    assert not n_links[po[:-1]].any() and not n_links[po[:-1] + 1].any()        # the frame has no links
    for name, (opt, box, dims, origin, spacing) in sd.LATTICES.items():
        lat = ld.Lattice(dims, origin, spacing)
        assert not ld.outside(xyz, lat).any()
        for brick in (4, 8):
            assert not ld.stray(xyz, lat, brick).any()
        # nodes with no, some and all images inactive (two images differ by image 0's thirds alone, which at spacing 16 reach
        # no node of their own)
        inactive = n_images - sd.active(lat, po, xyz).sum(axis=0)
        assert np.any(inactive == 0) and np.any(inactive == n_images), name
        assert np.any((inactive > 0) & (inactive < n_images)) or (name == "narrow" and n_images == 2), name
        # the slots of image 0's (and image 1's) bricks: the arms are whole bricks, of 5, 6 and 2 slots
        for image in (0, 1):
            sd.check_slots(xyz[po[image]:po[image + 1]], lat, name)
        for image in range(2, n_images):                        # nobody else has a brick of more than one slot
            assert po[image + 1] - po[image] <= sd.SCATTER_CHUNK
    assert 3375 % 16 != 0 and 729 % 4 != 0 and 729 < 2048


def test_the_count():
    c = np.zeros((2, 4, 3), np.float32)
    c[0, 1] = [1.0, -2.0, 3.0]; c[1, 3] = [-1.0, np.nextafter(np.float32(2), np.float32(3)), 0.0]
    assert sd.oversize(c, [1.0, 2.0, 3.0]) == 1                 # strictly beyond, per axis, by magnitude
    assert sd.oversize(c, [np.nextafter(1.0, 0), 2.0, 3.0]) == 3
    assert sd.oversize(c, [0.0, 0.0, 0.0]) == 5
    r, v, n = sd.boundary_ratio(c, 8.0, "max")
    assert v == 3.0 and n == 1 and float(r) * 8.0 == 3.0


@pytest.mark.parametrize("n_images,n_fixed", [(2, 0), (65, 0), (130, 0), (65, 1)])
def test_the_oracle_stays_inside_the_bound(n_images, n_fixed):
    """Two steps at alpha = 1 (the second from non-zero coefficients); with a fixed image no mean is removed, the fixed
    image's lattice stays zero and its points get no sums."""
    po, xyz, blocks = sd.build(n_images)
    ref, info = oracle_at(n_images, **({"n_fixed_images": n_fixed} if n_fixed else {}))
    lat = ld.Lattice.of(info)
    sd.check_frame(info, "wide", ref.xyz(), ref.xyz2(), xyz, n_images, n_fixed)
    n_links = sd.links_per_point(po, blocks)
    worst = 0.0
    for it in range(2):
        c_prev = coefficients(ref, n_images)
        x2 = ref.xyz2()
        assert sd.link_lengths(po, blocks, x2).max() < 0.095
        want_e = sd.energy(po, blocks, x2, n_fixed)
        e = ref.deformable_step(ALPHA)
        assert abs(e - want_e) <= 1e-6 * want_e, (e, want_e)
        if not n_fixed:
            assert abs(want_e - ld.energy(po, blocks, x2)[0]) <= 1e-12 * want_e
        sums = ref.point_sums()
        assert np.array_equal(sums[po[n_fixed]:, 3], n_links[po[n_fixed]:].astype(np.float32))
        r = ld.step(lat, po, ref.xyz(), sums, c_prev, ALPHA, mean_over=None if n_fixed else ld.ALL_IMAGES, first_image=n_fixed)
        assert np.all((r["gw"] == 0) | (r["gw"] >= 2.0 ** -140))     # the condition the bound is derived under
        c = coefficients(ref, n_images)
        assert not c[:n_fixed].any()
        ratio, at = ld.worst_ratio(r["new"], r["bound"], c[:, r["nodes"]])
        assert ratio <= 2.0, (it, ratio, at)
        worst = max(worst, ratio)
        if n_fixed:
            assert np.abs(c[n_fixed:].astype(np.float64).sum(axis=0)).max() > 1e-4      # no mean was removed
        ref.transform_points()
    assert float(np.abs(ref.xyz2().astype(np.float64) - xyz).max()) >= sd.MOVED      # the steps moved the points
    print(f"{n_images} images, {n_fixed} fixed: worst err / bound of the oracle {worst:.3f}")


def test_the_oracles_guard_at_the_limit():
    """The limit on an attained |coefficient| v (spacing 8: r = v / 8 is exact).  The step at r is judged by the strict count
    of the oracle's own coefficients -- v itself is not beyond the limit --, the step one float below r is rejected."""
    n = 65
    free, info = oracle_at(n)
    assert free.deformable_step(ALPHA) >= 0
    c = coefficients(free, n)
    for at in ("max", "median"):
        r, v, shared = sd.boundary_ratio(c, 8.0, at)
        below = np.nextafter(r, np.float32(0))
        n_at, n_below = sd.oversize(c, [float(r) * 8.0] * 3), sd.oversize(c, [float(below) * 8.0] * 3)
        assert n_below == n_at + shared and shared >= 1
        assert (n_at == 0) == (at == "max")
        for ratio, count in ((r, n_at), (below, n_below)):
            g, _ = oracle_at(n, guarantee_diffeomorphism=1, max_displacement_ratio=float(ratio))
            e = g.deformable_step(ALPHA)
            got = coefficients(g, n)
            if count:
                assert e == -1.0 and not got.any(), (at, float(ratio), e)
            else:
                assert e >= 0 and np.array_equal(got, c), (at, float(ratio), e)
