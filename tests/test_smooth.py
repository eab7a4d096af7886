"""The coverage-aware Gaussian without a device (frog_smooth_taps, frog_smooth_volume, frog_glm_smooth; include/frog_chain.h):
the library's taps against the restated formula, the two forms of the NumPy restatement (smooth_restate.py) against each other
and against scipy.ndimage, the invariants the header states, what the library refuses before it asks for a device, and the
designed case that shows what smoothing before the fit is for."""
import ctypes as C

import numpy as np
import pytest

from frog_amd import _abi
from frog_amd.volume import fwe_p, smooth_taps

import glm_restate as G
import smooth_restate as S

F4, F8, U4 = np.float32, np.float64, np.uint32


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(U4 if a.dtype == F4 else np.uint64), b.view(U4 if b.dtype == F4 else np.uint64))


# ---- 1. the taps ---------------------------------------------------------------------------------------------------------------

def test_taps_equal_the_restated_formula():
    """Two exponentials of 1 ulp each (the host libm's and NumPy's) differ by at most 2 ulp: 2^-51 relative."""
    for sigma, spacing in ((1.0, 1.0), (4.0 / S.FWHM, 1.0), (8.0 / S.FWHM, 0.7), (0.3, 1.5), (2.5, 0.12), (21.0, 1.0), (1e-3, 1.0), (1.0, 3.5)):
        R, w = smooth_taps(sigma, spacing)
        Rw, want = S.taps(sigma, spacing)
        assert R == Rw == len(w) - 1, (sigma, spacing)
        assert w[0] == 1.0 and w.dtype == F8
        assert (np.abs(w - want) <= 2.0 ** -51 * want).all(), (sigma, spacing)
        assert (np.diff(w) <= 0).all() and (w >= 0).all()


def test_radius_at_and_around_exact_multiples():
    """Where 3 sigma / s is an integer k the radius is k, and one ulp of sigma below it still k.  One ulp above, the rounded
    product decides: k + 1 where 3 sigma is representable beyond k (sigma = 1, 2 and 16: the product is exact), else what the
    two rounded operations give, which the restatement states."""
    for k, spacing in ((3, 1.0), (6, 1.0), (6, 0.5), (12, 0.25), (48, 1.0), (64, 1.0), (9, 2.0), (64, 0.75)):
        sigma = k * spacing / 3.0
        assert F8(3.0) * F8(sigma) / F8(spacing) == k                       # exact in f64 for these
        assert smooth_taps(sigma, spacing)[0] == k == S.radius(sigma, spacing)
        below = np.nextafter(sigma, 0.0)
        assert smooth_taps(below, spacing)[0] == S.radius(below, spacing) == k
        above = np.nextafter(sigma, np.inf)
        want = S.radius(above, spacing)
        assert want in (k, k + 1)
        if (k, spacing) in ((3, 1.0), (6, 1.0), (48, 1.0), (64, 0.75)):
            assert want == k + 1
        if want <= 64:
            assert smooth_taps(above, spacing)[0] == want
        else:
            with pytest.raises(_abi.FrogError) as e:
                smooth_taps(above, spacing)
            assert e.value.code == _abi.FROG_E_INVALID


# ---- 2. refusals that need no device ---------------------------------------------------------------------------------------------

def test_refusals_before_the_device_is_asked():
    """Each of these is FROG_E_INVALID also where there is no device, so none of them got as far as asking for one."""
    lib = _abi.hip_lib()
    r, w = C.c_uint32(), (C.c_double * 65)()
    assert lib.frog_smooth_taps(1.0, 1.0, C.byref(r), None) == _abi.FROG_OK and r.value == 3       # the radius alone
    for sigma, spacing in ((0.0, 1.0), (-1.0, 1.0), (np.nan, 1.0), (np.inf, 1.0), (1.0, 0.0), (1.0, -2.0), (1.0, np.nan), (1.0, np.inf),
                           (22.0, 1.0), (1.0, 0.04)):
        assert lib.frog_smooth_taps(sigma, spacing, C.byref(r), w) == _abi.FROG_E_INVALID, (sigma, spacing)
    assert lib.frog_smooth_taps(1.0, 1.0, None, w) == _abi.FROG_E_INVALID
    x = np.zeros((3, 4, 5), F4)
    out = np.empty(x.shape, F4)
    op = out.ctypes.data_as(_abi.c_float_p)
    v = _abi.volume_view(x, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    assert lib.frog_smooth_volume(None, None, 1.0, 0, op) == _abi.FROG_E_INVALID
    assert lib.frog_smooth_volume(C.byref(v), None, 1.0, 0, None) == _abi.FROG_E_INVALID
    for sigma in (-1.0, np.nan, np.inf, 22.0):
        assert lib.frog_smooth_volume(C.byref(v), None, sigma, 0, op) == _abi.FROG_E_INVALID, sigma
    thin = _abi.volume_view(x, (0.0, 0.0, 0.0), (1.0, 0.04, 1.0))               # a radius of 75 along y alone
    assert lib.frog_smooth_volume(C.byref(thin), None, 1.0, 0, op) == _abi.FROG_E_INVALID
    d = np.zeros((3, 4, 5), F8)
    assert lib.frog_smooth_volume(C.byref(_abi.volume_view(d, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))), None, 1.0, 0, op) == _abi.FROG_E_INVALID
    nodata = _abi.volume_view(None, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (5, 4, 3))
    assert lib.frog_smooth_volume(C.byref(nodata), None, 1.0, 0, op) == _abi.FROG_E_INVALID
    assert lib.frog_glm_smooth(None, 1.0) == _abi.FROG_E_INVALID
    planes = C.c_uint32()
    assert lib.frog_glm_smooth_planes(None, 4, 1.0, 0, C.byref(planes)) == _abi.FROG_E_INVALID
    assert lib.frog_glm_smooth_planes(C.byref(nodata), 4, 1.0, 0, None) == _abi.FROG_E_INVALID
    for sigma in (-1.0, np.nan, np.inf, 22.0):
        assert lib.frog_glm_smooth_planes(C.byref(nodata), 4, sigma, 0, C.byref(planes)) == _abi.FROG_E_INVALID, sigma
    assert lib.frog_glm_smooth_planes(C.byref(nodata), 4097, 1.0, 0, C.byref(planes)) == _abi.FROG_E_INVALID


# ---- 3. the restatement ------------------------------------------------------------------------------------------------------------

def holes(rng, shape, share=0.3):
    on = rng.random(shape) >= share
    on[:, 1, :] = False                                         # a whole row of every plane
    on[1] = False                                               # a whole plane
    return on


def test_the_two_forms_of_the_restatement_agree():
    rng = np.random.default_rng(3)
    for shape, sigma, spacing in (((4, 5, 6), 1.0, (1.0, 1.0, 1.0)), ((3, 4, 7), 0.8, (0.5, 1.0, 2.0)), ((2, 3, 5), 0.3, (1.0, 1.0, 1.0))):
        x = rng.normal(0, 1, shape).astype(F4)
        x[0, 0, 0], x[-1, -1, -1], x[0, 2, 1], x[0, 0, 2] = np.inf, np.nan, F4(-0.0), F4(3e38)
        on = S.taking(x, holes(rng, shape))
        w3 = [S.taps(sigma, s)[1] for s in spacing]
        a, b = S.smooth(x, on, w3), S.literal(x, on, w3)
        assert same(a, b), shape
        assert (np.isnan(a) == ~on).all() and on.any() and not on.all()


def test_restatement_against_scipy():
    """correlate1d sums in another order: the f64 fields agree within 2^-40 relative, far above f64's rounding of these sums
    of positive terms (the values lie around 10: nothing cancels) and far below any mistake in a tap or an index."""
    from scipy.ndimage import correlate1d
    rng = np.random.default_rng(8)
    for shape, sigma, spacing in (((9, 11, 13), 1.0, (1.0, 1.0, 1.0)), ((7, 6, 10), 1.4, (0.5, 1.0, 2.0)), ((5, 4, 3), 2.0, (1.0, 1.0, 1.0))):
        x = (10 + rng.normal(0, 1, shape)).astype(F4)
        on = holes(rng, shape)
        w3 = [S.taps(sigma, s)[1] for s in spacing]
        got, got_num, got_den = S.smooth(x, on, w3, fields=True)
        num, den = np.where(on, x, 0).astype(F8), on.astype(F8)
        for axis, w in ((2, w3[0]), (1, w3[1]), (0, w3[2])):
            full = np.concatenate([w[:0:-1], w])
            num, den = (correlate1d(f, full, axis=axis, mode="constant", cval=0.0) for f in (num, den))
        assert (den[on] >= 1).all() and (got_den[on] >= 1).all()
        assert (np.abs(got_num - num) <= 2.0 ** -40 * num).all() and (np.abs(got_den - den) <= 2.0 ** -40 * den).all(), shape
        want = num[on] / den[on]
        assert (np.abs(got_num[on] / got_den[on] - want) <= 2.0 ** -40 * want).all(), shape
        assert same(got[on], (got_num[on] / got_den[on]).astype(F4)) and (got.view(U4)[~on] == U4(0x7FC00000)).all()


def test_invariants():
    rng = np.random.default_rng(12)
    shape = (8, 9, 10)
    on = holes(rng, shape, 0.4)
    on[5:8, 5:9, 5:10] = False
    on[6, 7, 8] = True                                          # alone: no participating neighbour within the radius of 1
    on[6:8, 7:9, 0:2] = False
    on[7, 8, 0] = True                                          # alone in a corner: its cube of 2 x 2 x 2 holds nobody else
    w3 = [S.taps(0.3, 1.0)[1]] * 3                              # radius 1
    assert len(w3[0]) == 2
    c = F4(0.1)                                                 # not a dyadic rational: num / den rounds
    out = S.smooth(np.full(shape, c, F4), on, w3)
    assert (np.isnan(out) == ~on).all()                         # the participating set is unchanged
    assert (np.abs(out[on].astype(F8) - F8(c)) <= 2.0 ** -52 * F8(c)).all()
    assert out[6, 7, 8] == c and out[7, 8, 0] == c
    x = rng.normal(0, 1, shape).astype(F4)
    out = S.smooth(x, on, w3)
    assert out[6, 7, 8] == x[6, 7, 8] and out[7, 8, 0] == x[7, 8, 0]            # kept exactly
    assert (np.isnan(out) == ~on).all() and not same(out[on], x[on])
    wide = [S.taps(2.0, 1.0)[1]] * 3
    out = S.smooth(np.full(shape, c, F4), on, wide)
    assert (np.abs(out[on].astype(F8) - F8(c)) <= 2.0 ** -52 * F8(c)).all()


# ---- 4. the designed case ----------------------------------------------------------------------------------------------------------

DESIGNED_GRID = ((24, 20, 16), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
DESIGNED_PERMS, DESIGNED_SEED, DESIGNED_SIGMA = 200, 4, 1.0
# what seed 31 gives: (block, outside) unsmoothed, then with sigma = 1 mm -- 2 and 461 of the block's 512 voxels, 0 and 7 of
# the 7168 others
DESIGNED_SHARES = ((2 / 512, 0.0), (461 / 512, 7 / 7168))


def designed_case():
    """20 images of N(0, 1) noise (f32) on the 16 x 20 x 24 (z, y, x) grid at 1 mm, alternating groups, +1.0 in group 1 inside
    the 8 x 8 x 8 block [4:12, 6:14, 8:16], 15 % of the entries missing at random.  Returns (volumes, on-grid masks uint8, design
    of an intercept and the group, the contrast on the group, block bool)."""
    rng = np.random.default_rng(31)
    n, shape = 20, DESIGNED_GRID[0][::-1]
    group = np.arange(n) % 2
    X = np.stack([np.ones(n), group.astype(F8)], axis=1)
    vols = rng.normal(0, 1, (n,) + shape).astype(F4)
    block = np.zeros(shape, bool)
    block[4:12, 6:14, 8:16] = True
    vols[group == 1] += np.where(block, F4(1), F4(0))
    on = (rng.random((n,) + shape) >= 0.15).astype(np.uint8)
    return vols, on, X, np.array([[0.0, 1.0]]), block


def shares(p, block):
    return float((p[block] < 0.05).mean()), float((p[~block] < 0.05).mean())


def designed_shares(planes, X, con, block):
    """(share of the block's voxels with a corrected p < 0.05, share of the others) of stored planes, on the restatement."""
    _, _, t, _, fit = G.finish(planes, X, con)
    perm, _ = G.draw(len(X), DESIGNED_PERMS, DESIGNED_SEED)
    hi, _ = G.permute(planes, X, con, perm, None, 2)
    return shares(fwe_p(t[0], hi[:, 0], fit=fit), block)


def designed_condition(raw, smoothed):
    """What the issue sets: unsmoothed fewer than 5 % of the block's voxels reach a corrected p < 0.05, with sigma = 1 mm
    more than 50 % do, and fewer than 1 % of the voxels outside the block."""
    assert raw[0] < 0.05, raw
    assert smoothed[0] > 0.50, smoothed
    assert smoothed[1] < 0.01, smoothed


def test_designed_case_on_the_restatement():
    """Seed 31 gives, of the block's voxels, 0.39 % unsmoothed and 90.04 % with sigma = 1 mm, and 0.098 % of the voxels outside
    it: DESIGNED_SHARES, which tests/test_gpu_smooth.py expects of the device to the last voxel.  The taps are the library's
    (host code), as on the device."""
    vols, on, X, con, block = designed_case()
    assert block.sum() == 512
    planes = np.where(on != 0, vols, G.NAN)
    w3 = [smooth_taps(DESIGNED_SIGMA, 1.0)[1]] * 3
    smoothed = S.smooth_planes(planes, w3)
    assert (np.isnan(smoothed) == np.isnan(planes)).all()
    raw_shares, smooth_shares = designed_shares(planes, X, con, block), designed_shares(smoothed, X, con, block)
    print("designed case: unsmoothed", raw_shares, "smoothed", smooth_shares)
    designed_condition(raw_shares, smooth_shares)
    assert (raw_shares, smooth_shares) == DESIGNED_SHARES
