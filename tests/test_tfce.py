"""The NumPy restatement of threshold-free cluster enhancement (tfce_restate.py; include/frog_chain.h states the semantics)
against closed forms that do not go through it: sums written out in Python floats, levels by Python's own correctly rounded
division, and scipy.ndimage.label for the components.  Every comparison is == on bytes."""
import math

import numpy as np
import pytest

import tfce_restate as T

F4, F8 = np.float32, np.float64
DHS = (0.25, 0.1)                                           # a power of two, and a step that is not a binary fraction


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def weight(k, dh, h):
    """w_k in Python floats (f64): the products one by one."""
    d = float(F4(dh))
    hk = float(k) * d
    return (hk * hk if h == 2 else hk) * d


def closed(extents, dh, e, h):
    """(float32) of the descending sum of g(extent_k) * w_k, extents = {k: extent at level k} for k = top..1."""
    acc = 0.0
    for k in sorted(extents, reverse=True):
        g = math.sqrt(float(extents[k])) if e == 0.5 else float(extents[k])
        m = g * weight(k, dh, h)
        acc = acc + m
    return F4(acc)


def mid(c, dh):
    """A statistic in the middle of level c."""
    return F4((c + 0.5) * dh)


@pytest.mark.parametrize("dh", DHS)
@pytest.mark.parametrize("e", (0.5, 1))
@pytest.mark.parametrize("h", (1, 2))
def test_a_box_alone_in_the_grid(dh, e, h):
    t = np.zeros((5, 6, 9), F4)
    t[1:3, 2:5, 3:7] = mid(7, dh)                           # 24 voxels at level 7
    got, top = T.tfce(t, dh, e, h)
    want = closed({k: 24 for k in range(1, 8)}, dh, e, h)
    assert (got[1:3, 2:5, 3:7] == want).all() and top == want and want > 0
    assert (got[t == 0] == 0).all() and got.dtype == F4


@pytest.mark.parametrize("dh", DHS)
@pytest.mark.parametrize("e", (0.5, 1))
@pytest.mark.parametrize("h", (1, 2))
def test_two_peaks_on_a_shared_plateau(dh, e, h):
    t = np.zeros((3, 5, 16), F4)
    t[1, 1:4, 2:14] = mid(3, dh)                            # the plateau: 36 voxels at level 3
    t[1, 2, 3:5] = mid(6, dh)                               # a peak of 2 voxels at level 6
    t[1, 2, 9:12] = mid(5, dh)                              # a peak of 3 voxels at level 5
    got, top = T.tfce(t, dh, e, h)
    plateau = {k: 36 for k in (1, 2, 3)}
    first = {**plateau, 4: 2, 5: 2, 6: 2}
    second = {**plateau, 4: 3, 5: 3}
    assert (got[1, 2, 3:5] == closed(first, dh, e, h)).all() and (got[1, 2, 9:12] == closed(second, dh, e, h)).all()
    rest = t == mid(3, dh)
    assert (got[rest] == closed(plateau, dh, e, h)).all() and (got[t == 0] == 0).all()
    assert top == max(closed(first, dh, e, h), closed(second, dh, e, h))


def python_level(t, dh, side=0):
    t, dh = float(F4(t)), float(F4(dh))
    s = -t if side else t
    if math.isnan(t) or s <= 0:
        return 0
    q = s / dh if not math.isinf(s) else math.inf           # Python's float division: one correctly rounded f64 division
    return 255 if q >= 255 else int(q)


def edge_values(dh):
    """k * dh as f32 and its two neighbours, values at and beyond 255 * dh, the zeros, negatives, infinities and the NaN."""
    d = F8(F4(dh))
    exact = (np.arange(0, 258, dtype=F8) * d).astype(F4)
    below, above = np.nextafter(exact, F4(-np.inf)), np.nextafter(exact, F4(np.inf))
    extra = np.array([0.0, -0.0, -1.0, -dh, 1e30, np.inf, -np.inf, np.nan, 254.999 * dh, 255.0 * dh, 300.0 * dh], F4)
    return np.concatenate([exact, below, above, extra])


@pytest.mark.parametrize("dh", DHS + (0.3, 1e-3, 7.0))
def test_levels_at_the_edges(dh):
    v = edge_values(dh)
    for side in (0, 1):
        got = T.levels(v, dh, side)
        want = np.array([python_level(x, dh, side) for x in v], np.uint8)
        assert same(got, want)
    top = T.levels(v, dh, 0)
    assert top.max() == 255 and (top[np.isnan(v)] == 0).all() and (top[v <= 0] == 0).all() and top[v == np.inf][0] == 255
    if dh == 0.25:                                          # exact arithmetic: k * dh is level k, one ulp below is k - 1
        assert same(top[:258], np.minimum(np.arange(258), 255).astype(np.uint8))
        assert same(top[259:516], np.minimum(np.arange(258)[1:] - 1, 255).astype(np.uint8))


def noise(shape, seed, df=10):
    return np.random.default_rng(seed).standard_t(df, shape).astype(F4)


@pytest.mark.parametrize("connectivity", (6, 18, 26))
def test_side_1_of_t_is_side_0_of_minus_t(connectivity):
    t = noise((4, 7, 13), 3)
    t[0, 0, :3] = (np.nan, 0.0, -0.0)
    a, top_a = T.tfce(t, 0.1, connectivity=connectivity, side=1)
    b, top_b = T.tfce(-t, 0.1, connectivity=connectivity, side=0)
    assert same(a, b) and top_a == top_b and top_a > 0
    pos = T.tfce(t, 0.1, connectivity=connectivity, side=0)[0]
    assert not ((pos > 0) & (a > 0)).any()                  # a voxel has at most one side


def test_tfce_p_against_a_hand_count():
    null = np.array([9.0, 1.0, 4.0, 4.0, 2.5, 0.0, 7.0, 3.0], F4)       # row 0 is the observed maximum: it does not count
    values = np.array([0.0, 0.5, 1.0, 2.5, 2.6, 4.0, 7.0, 7.5, 9.0, -4.0, -0.0], F4)
    #                   0    >=: 6    6    5    4    3    1    0    0    3     0
    want = np.array([1.0] + [(1 + n) / 8.0 for n in (6, 6, 5, 4, 3, 1, 0, 0, 3)] + [1.0], F8).astype(F4)
    assert same(T.tfce_p(values, null), want)
    from frog_amd.volume import tfce_p
    assert same(tfce_p(values, null), want)
    assert same(tfce_p(values.reshape(1, 11), null), want.reshape(1, 11))


def scipy_tfce(t, dh, e, h, connectivity, side=0):
    """The same sum with scipy.ndimage.label for the components and the levels from python_level."""
    from scipy import ndimage
    structure = ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity])
    level = np.array([python_level(x, dh, side) for x in t.reshape(-1)], np.int64).reshape(t.shape)
    acc = np.zeros(t.shape, F8)
    for k in range(int(level.max()), 0, -1):
        labels, n = ndimage.label(level >= k, structure)
        extent = np.bincount(labels.reshape(-1), minlength=n + 1).astype(F8)
        g = np.sqrt(extent) if e == 0.5 else extent
        m = g[labels] * weight(k, dh, h)
        acc = np.where(level >= k, acc + m, acc)
    return acc.astype(F4)


@pytest.mark.parametrize("connectivity,e,h,dh", [(26, 0.5, 2, 0.1), (6, 1, 1, 0.1), (18, 0.5, 1, 0.25), (26, 1, 2, 0.3), (6, 0.5, 2, 0.25)])
def test_restatement_equals_scipy(connectivity, e, h, dh):
    pytest.importorskip("scipy.ndimage")
    t = noise((6, 9, 14), 11 + connectivity)
    t[2:4, 3:6, 4:9] += F4(2.0)                             # a broad, weak region among the noise
    for side in (0, 1):
        got = T.tfce(t, dh, e, h, connectivity, side)[0]
        assert same(got, scipy_tfce(t, dh, e, h, connectivity, side)) and got.max() > 0
