"""The NumPy restatement of the surface distances (surface_restate.py; include/frog_chain.h states the arithmetic) on
designed geometry with known answers, its two brute forces against each other, and the refusals of the Python wrappers that
need no device."""
import numpy as np
import pytest

from frog_amd import _abi
from frog_amd.volume import SURFACE_ROW, SurfaceDistances, distance_map, surface_metrics

import surface_restate as sr

SHAPE = (7, 13, 19)                                         # [z, y, x] of the 19 x 13 x 7 grid
UNIT = 65536


def box(x0, x1, y0=3, y1=9, z0=2, z1=5, shape=SHAPE, value=58):
    m = np.zeros(shape, np.uint8)
    m[z0:z1, y0:y1, x0:x1] = value
    return m


def test_shifted_box_has_the_shift_as_its_hausdorff_distance():
    reference, image = box(4, 10), box(6, 12)
    r = sr.rows(image, reference, [58], (1.5, 1.0, 1.0))
    h, hp, assd = sr.metrics(r)
    assert h[0] == 3.0 and r["max_ab"][0] == r["max_ba"][0] == 3 * UNIT
    assert r["n_a"][0] == r["n_b"][0] == int(sr.surface(image, 58).sum())
    assert 0 < assd[0] < 3.0 and hp[0] == 3.0
    assert r["sum_ab"][0] == r["sum_ba"][0]                 # the two maps are mirror images of each other


def test_identical_maps_are_at_distance_zero():
    m = box(4, 10)
    r = sr.rows(m, m, [58], (0.7, 1.3, 2.1))[0]
    assert r["n_a"] == r["n_b"] > 0
    assert all(r[k] == 0 for k in ("sum_ab", "sum_ba", "max_ab", "max_ba", "pct_ab", "pct_ba"))
    assert [float(x[0]) for x in sr.metrics(r)] == [0.0, 0.0, 0.0]


def test_single_voxels():
    a, b = np.zeros(SHAPE, np.int16), np.zeros(SHAPE, np.int16)
    a[1, 2, 3] = -3
    b[4, 6, 6] = -3                                         # (3, 4, 3) voxels away: 3-4-5 in the xy plane at unit spacing
    r = sr.rows(a, b, [-3], (1.0, 1.0, 1.0))[0]
    d = int(np.rint(np.sqrt(34.0) * UNIT))
    assert (r["n_a"], r["n_b"]) == (1, 1)
    assert all(r[k] == d for k in ("sum_ab", "sum_ba", "max_ab", "max_ba", "pct_ab", "pct_ba"))
    r = sr.rows(a, b, [-3], (1.0, 1.0, 0.0625))[0]          # dz = 3/16: 25 + 9/256 is exact
    assert r["max_ab"] == int(np.rint(np.sqrt(25.0 + 9.0 / 256.0) * UNIT))
    m = sr.distance_map(a, -3, (2.0, 1.0, 1.0), 0)
    assert m[1, 2, 3] == 0 and m[1, 2, 0] == 6 * UNIT and m[1, 0, 3] == 2 * UNIT and m[0, 2, 3] == UNIT


def test_a_structure_on_the_border_has_surface_there():
    m = np.full(SHAPE, 58, np.uint8)
    s = sr.surface(m, 58)
    inner = np.zeros(SHAPE, bool)
    inner[1:-1, 1:-1, 1:-1] = True
    assert (s == ~inner).all()
    assert not sr.surface(box(4, 10), 58)[3, 5, 6] and sr.surface(box(4, 10), 58)[2, 5, 6]
    flush = box(0, 5)                                       # cut by the border at x = 0
    assert sr.surface(flush, 58)[3, 5, 0] and not sr.surface(flush, 58)[3, 5, 1]
    other = flush.copy()
    other[3, 5, 2] = 86                                     # another label inside: its neighbours become surface
    assert sr.surface(other, 58)[3, 5, 1] and sr.surface(other, 58)[3, 5, 3] and sr.surface(other, 86)[3, 5, 2]


def test_an_absent_label_gives_the_sentinel_row_and_nan():
    m = box(4, 10)
    r = sr.rows(m, m, [58, 86], (1.0, 1.0, 1.0))
    assert (r["n_a"][1], r["n_b"][1], r["sum_ab"][1], r["sum_ba"][1]) == (0, 0, 0, 0)
    assert all(r[k][1] == 0xFFFFFFFF for k in ("max_ab", "max_ba", "pct_ab", "pct_ba"))
    half = sr.rows(np.where(m == 58, 86, 0).astype(np.uint8), m, [58, 86], (1.0, 1.0, 1.0))
    assert (half["n_a"][0], half["n_b"][0]) == (0, r["n_b"][0]) and (half["n_a"][1], half["n_b"][1]) == (r["n_a"][0], 0)
    assert all(half[k][l] == 0xFFFFFFFF for k in ("max_ab", "max_ba", "pct_ab", "pct_ba") for l in (0, 1))
    for got in (sr.metrics(half), surface_metrics(half.astype(SURFACE_ROW))):
        assert all(np.isnan(x).all() for x in got)
    assert (sr.distance_map(m, 86, (1.0, 1.0, 1.0), 0) == 0xFFFFFFFF).all()
    h, hp, assd = surface_metrics(r.astype(SURFACE_ROW))
    assert h[0] == hp[0] == assd[0] == 0.0 and np.isnan([h[1], hp[1], assd[1]]).all()


def test_the_rank_of_the_percentile():
    assert [sr.kth(n, 95) for n in (1, 20, 21, 100, 101)] == [1, 19, 20, 95, 96]
    assert [sr.kth(n, 100) for n in (1, 20, 21, 100, 101)] == [1, 20, 21, 100, 101]
    assert [sr.kth(n, 1) for n in (1, 20, 21, 100, 101)] == [1, 1, 1, 1, 2]
    reference, image = box(4, 10), box(6, 12)
    top = sr.rows(image, reference, [58], (1.0, 1.0, 1.0), 100)[0]
    assert top["pct_ab"] == top["max_ab"] and top["pct_ba"] == top["max_ba"]
    low = sr.rows(image, reference, [58], (1.0, 1.0, 1.0), 1)[0]
    assert low["pct_ab"] == 0 and low["pct_ba"] == 0        # the overlapping faces touch


@pytest.mark.parametrize("spacing", [(1.0, 1.0, 1.0), (0.5, 2.0, 1.25), (0.25, 0.125, 4.0)])
def test_the_separable_restatement_is_the_brute_force_at_dyadic_spacings(spacing):
    rng = np.random.default_rng(5)
    for density in (0.02, 0.5):
        f = rng.random(SHAPE) < density
        assert np.array_equal(sr.squared_distance(f, spacing), sr.brute_force_squared_distance(f, spacing))
    assert np.isinf(sr.brute_force_squared_distance(np.zeros(SHAPE, bool), spacing)).all()
    assert np.isinf(sr.squared_distance(np.zeros(SHAPE, bool), spacing)).all()


def test_the_two_restatements_within_one_unit_at_a_spacing_that_rounds():
    rng = np.random.default_rng(7)
    spacing = (0.7, 1.3, 2.1)
    for density in (0.02, 0.5):
        f = rng.random(SHAPE) < density
        a, b = sr.fixed(sr.squared_distance(f, spacing)), sr.fixed(sr.brute_force_squared_distance(f, spacing))
        assert np.abs(a.astype(np.int64) - b.astype(np.int64)).max() <= 1


def test_surface_metrics_is_the_restatement():
    rng = np.random.default_rng(9)
    image = rng.choice([0, 58, 86], size=SHAPE).astype(np.uint8)
    reference = rng.choice([0, 58, 86, 170], size=SHAPE).astype(np.uint8)
    r = sr.rows(image, reference, [58, 86, 170], (0.7, 1.3, 2.1))
    for got, want in zip(surface_metrics(r.astype(SURFACE_ROW)), sr.metrics(r)):
        assert got.dtype == np.float64 and np.array_equal(got, want, equal_nan=True)
    assert r["n_a"][2] == 0 and r["n_b"][2] > 0


def invalid(call, *args, **kw):
    with pytest.raises(_abi.FrogError) as e:
        call(*args, **kw)
    assert e.value.code == _abi.FROG_E_INVALID, str(e.value)


def test_the_wrappers_refuse_before_any_device_use():
    m = box(4, 10)
    invalid(distance_map, m.astype(np.float32), 58)
    invalid(distance_map, m.astype(np.float64), 58)
    invalid(distance_map, m, 58, mode=2)
    invalid(distance_map, m, 58, mode=-1)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        invalid(distance_map, m, 58, spacing=(1.0, bad, 1.0))
        invalid(SurfaceDistances, m, [58], (bad, 1.0, 1.0))
    invalid(distance_map, np.zeros((0, 3, 3), np.uint8), 58)
    with pytest.raises(ValueError):
        distance_map(m[0], 58)
    invalid(SurfaceDistances, m.astype(np.float32), [58])
    invalid(SurfaceDistances, m, [])
    invalid(SurfaceDistances, m, list(range(_abi.FROG_SURFACE_MAX_LABELS + 1)))
    invalid(SurfaceDistances, m, [58, 58])
    invalid(SurfaceDistances, m, [86, 58])
    invalid(SurfaceDistances, m, [58, -3])                  # ascending as signed values
    invalid(SurfaceDistances, m, [58], (1.0, 1.0, 1.0), 0)
    invalid(SurfaceDistances, m, [58], (1.0, 1.0, 1.0), 101)
    with pytest.raises(ValueError):
        SurfaceDistances(m, [58], (1.0, 1.0, 1.0), -1)
    with pytest.raises(ValueError):
        SurfaceDistances(m, [58], ((19, 13, 8), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)))
