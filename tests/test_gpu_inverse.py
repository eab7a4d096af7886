"""The Newton inverse of a B-spline link (bspline_inverse, frog_amd/csrc/device/chain.hip) on strong, composed and folded
lattices, against tests/inverse_restate.py: a NumPy restatement of the forward link and a plain Newton polish, not the
oracle's restatement of the same algorithm.  tests/test_chain.py makes the same assertions of the oracle.

The figures worth keeping (the device's distance to the oracle, its unsolved share on the folded lattice) are kept
as inverse_* where gpu_util.note keeps a GPU run's numbers: recorded, not asserted.  See DESIGN.md, "Inverse chains and volume reslicing"."""
import numpy as np
import pytest

import inverse_restate as ir
from field_restate import node_list
from frog_amd.chain import Chain, invert
from oracle.oracle_api import chain_apply
from gpu_util import note as record

pytestmark = pytest.mark.gpu


def keep(name, value):
    record("inverse_" + name, value)


def device_apply(links, points):
    c = Chain(list(links))
    try:
        return c.apply(points)
    finally:
        c.close()


def test_strong_lattice_converges_onto_the_root():
    x = ir.check_strong(device_apply, keep)
    link, p = ir.strong_lattice(ir.STRONG_FRAC), ir.sample_points(5)
    apart = np.linalg.norm(x - chain_apply([ir.inverse_link(link)], p), axis=1).max()
    keep("strong_max_device_to_oracle", apart)
    assert apart <= ir.PAIR_DISTANCE        # both within ROOT_DISTANCE of the one root; a shortened point may take another branch


def test_inverted_pyramid_is_its_links_one_at_a_time():
    p, x = ir.check_stages(device_apply, invert(list(ir.pyramid_chain())))
    ir.check_round_trip(p, x, keep)


def test_jacobian_of_the_inverse_is_the_inverse_at_the_returned_point():
    inv = invert(list(ir.pyramid_chain()))
    grid = ir.JACOBIAN_GRID
    nodes = node_list(*grid)
    c = Chain(inv)
    disp, det = c.sample(*grid, dtype=np.float64)
    only_disp, none = c.sample(*grid, determinant=False, dtype=np.float64)
    n, m = c.check(*grid)
    x = c.apply(nodes)
    c.close()
    assert none is None and disp.tobytes() == only_disp.tobytes()       # chain_point<true> and <false> walk the same points
    assert (x - nodes).tobytes() == disp.tobytes()
    product = det.ravel() * ir.stage_determinant(device_apply, inv, nodes)
    keep("jacobian_max_product_error", np.abs(product - 1).max())
    assert np.abs(product - 1).max() < 1e-9
    assert n == 0 and m == det.min()


def test_folded_lattice_ends_at_a_point_no_worse_than_the_first_guess():
    ir.check_folded(device_apply, keep)


def test_non_finite_points_return_as_the_oracle_has_them():
    pts = ir.non_finite_points()
    for links in ([ir.inverse_link(ir.strong_lattice(ir.STRONG_FRAC))], invert(list(ir.pyramid_chain()))):
        got, want = device_apply(links, pts), chain_apply(links, pts)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isfinite(got), np.isfinite(want))
        ok = np.isfinite(want)
        if ok.any():
            assert np.abs(got[ok] - want[ok]).max() <= 1e-12
