"""frog_rank without a device: its NumPy restatement (rank_restate.py) against np.quantile and np.median, the sort-key map,
and every refusal of include/frog_chain.h that needs no accumulator."""
import ctypes as C

import numpy as np
import pytest

from frog_amd import _abi

import rank_restate

F4, U4 = np.float32, np.uint32
EXACT_Q = (0.0, 0.25, 0.5, 0.75, 1.0, 0.05, 0.95)


def bits(a):
    return np.ascontiguousarray(a, F4).view(U4)


@pytest.mark.parametrize("n", range(1, 40))
def test_restatement_equals_numpy_quantile_and_median(n):
    """Integer-valued data below 2^20: every product and sum of the linear rule is exact in float64 for these q."""
    rng = np.random.default_rng(100 + n)
    x = rng.integers(-(1 << 20) + 1, 1 << 20, (n, 3, 4, 5)).astype(F4)
    x[:, 0, 0, 0] = x[0, 0, 0, 0]                                           # one voxel where all agree
    planes = rank_restate.entries(x, np.ones(x.shape, bool))
    values, mad, count = rank_restate.finish(planes, quantiles=EXACT_Q)
    assert (count == n).all() and count.dtype == np.uint16
    for j, q in enumerate(EXACT_Q):
        want = np.quantile(x.astype(np.float64), q, axis=0, method="linear").astype(F4)
        assert np.array_equal(bits(values[j]), bits(want)), q
    med = np.median(x.astype(np.float64), axis=0).astype(F4)
    assert np.array_equal(bits(values[2]), bits(med))
    want_mad = np.median(np.abs(x - med[None]).astype(np.float64), axis=0).astype(F4)
    assert np.array_equal(bits(mad), bits(want_mad))
    assert values[2][0, 0, 0] == x[0, 0, 0, 0] and mad[0, 0, 0] == 0


def test_restatement_counts_fills_and_skips():
    """k varies per voxel: NaNs and invalid entries do not take part; below min_count the fill and a zero MAD."""
    rng = np.random.default_rng(7)
    x = rng.integers(-50, 50, (9, 6, 5, 4)).astype(F4)
    valid = rng.random(x.shape) < 0.6
    x[rng.random(x.shape) < 0.1] = np.nan
    part = valid & ~np.isnan(x)
    values, mad, count = rank_restate.finish(rank_restate.entries(x, valid), min_count=3, fill=-7.5, quantiles=(0.5, 1.0))
    assert np.array_equal(count, part.sum(axis=0)) and count.min() < 3 < count.max()
    for idx in np.ndindex(x.shape[1:]):
        v = x[(slice(None),) + idx][part[(slice(None),) + idx]]
        if len(v) < 3:
            assert values[0][idx] == F4(-7.5) and values[1][idx] == F4(-7.5) and mad[idx] == 0
        else:
            assert values[0][idx] == F4(np.median(v.astype(np.float64))) and values[1][idx] == v.max()
            assert mad[idx] == F4(np.median(np.abs(v - values[0][idx]).astype(np.float64)))


def test_infinite_neighbours():
    """Equal infinite neighbours give themselves (no inf - inf); -inf next to +inf gives the quiet NaN, and so does its MAD."""
    inf = F4(np.inf)
    cols = [[-inf, -inf, 1, 2], [1, 2, inf, inf], [-inf, -inf, inf, inf], [-inf, 0, 0, inf], [-0.0, -0.0, 0.0, 0.0]]
    x = np.array(cols, F4).T.reshape(4, 5, 1, 1)
    values, mad, _ = rank_restate.finish(rank_restate.entries(x, np.ones(x.shape, bool)), quantiles=(0.25, 0.5, 0.75))
    v = values[:, :, 0, 0]
    assert v[0, 0] == -inf and v[2, 1] == inf and v[0, 2] == -inf and v[2, 2] == inf
    assert bits(v[1, 2]) == 0x7FC00000 and bits(mad[2, 0, 0]) == 0x7FC00000
    assert v[1, 3] == 0 and mad[3, 0, 0] == inf                               # distances 0, 0, inf, inf
    assert bits(v[1, 4]) == 0x80000000 and mad[4, 0, 0] == 0                # -0 == +0: the lower neighbour as it is
    assert bits(mad[0, 0, 0]) == 0x7FC00000                                 # the median -inf .. 1 is -inf: not finite


def test_key_map_is_strictly_increasing_and_keeps_the_sentinel_free():
    tiny = np.array([1], U4).view(F4)[0]
    ladder = np.array([-np.inf, -3.5, -tiny, -0.0, 0.0, tiny, 2.0, np.inf], F4)
    keys = rank_restate.keys_of(ladder).astype(np.int64)
    assert (np.diff(keys) > 0).all()
    assert np.array_equal(bits(rank_restate.values_of(rank_restate.keys_of(ladder))), bits(ladder))
    # the only bit patterns that map to 0xFFFFFFFF: u with ~u = 0xFFFFFFFF has no sign bit; u ^ 0x80000000 = 0xFFFFFFFF is
    # 0x7FFFFFFF, a NaN.  Checked over every exponent-all-ones pattern and a sweep of the rest.
    u = np.concatenate([np.arange(0x7F800000, 0x80000000, dtype=np.uint64), np.arange(0xFF800000, 0x100000000, dtype=np.uint64),
                        np.arange(0, 0x100000000, 4099, dtype=np.uint64)]).astype(U4)
    hit = u[rank_restate.keys_of(u.view(F4)) == rank_restate.SENTINEL]
    assert hit.tolist() == [0x7FFFFFFF] and np.isnan(hit.view(F4)).all()
    assert (rank_restate.keys_of(np.array([np.inf], F4)) < rank_restate.SENTINEL).all()


def grid_view(dims):
    return _abi.volume_view(None, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), dims)


def test_refusals_come_before_device_use():
    """FROG_E_INVALID whether or not a device is present: what needs no accumulator."""
    lib = _abi.hip_lib()
    INVALID = _abi.FROG_E_INVALID
    g, planes, h = grid_view((7, 5, 3)), C.c_uint32(), C.c_void_p()
    # NULL arguments
    assert lib.frog_rank_planes(None, 5, 0, C.byref(planes)) == INVALID
    assert lib.frog_rank_planes(C.byref(g), 5, 0, None) == INVALID
    assert lib.frog_rank_create(None, 0, 3, 5, 0, C.byref(h)) == INVALID
    assert lib.frog_rank_create(C.byref(g), 0, 3, 5, 0, None) == INVALID
    assert lib.frog_rank_add(None, None, C.byref(g), None, 1, 0.0) == INVALID
    q = (C.c_double * 1)(0.5)
    out = np.empty(105, F4)
    assert lib.frog_rank_finish(None, 1, 0.0, 1, q, out.ctypes.data_as(_abi.c_float_p), None, None) == INVALID
    # an empty grid, one above 2^31 voxels
    for dims in ((0, 5, 3), (7, 5, 0), (2048, 2048, 513)):
        e = grid_view(dims)
        assert lib.frog_rank_planes(C.byref(e), 5, 0, C.byref(planes)) == INVALID, dims
        assert lib.frog_rank_create(C.byref(e), 0, 1, 5, 0, C.byref(h)) == INVALID, dims
    # a window outside the grid, no planes
    for first, n in ((3, 1), (0, 4), (2, 2), (0, 0), (0xFFFFFFFF, 2)):
        assert lib.frog_rank_create(C.byref(g), first, n, 5, 0, C.byref(h)) == INVALID, (first, n)
    # no images, more than the capacity
    assert _abi.FROG_RANK_MAX_IMAGES >= 4096
    for n in (0, _abi.FROG_RANK_MAX_IMAGES + 1):
        assert lib.frog_rank_planes(C.byref(g), n, 0, C.byref(planes)) == INVALID, n
        assert lib.frog_rank_create(C.byref(g), 0, 3, n, 0, C.byref(h)) == INVALID, n
    assert not h.value
    # valid arguments reach the device: a result, or the refusal to run without one
    rc = lib.frog_rank_planes(C.byref(g), _abi.FROG_RANK_MAX_IMAGES, 0, C.byref(planes))
    assert rc == (_abi.FROG_OK if lib.frog_device_count() > 0 else _abi.FROG_E_NODEVICE)
