"""frog_glm without a device (include/frog_chain.h): the NumPy restatement (glm_restate.py) against independent code, its
two forms against each other, frog_glm_draw against its restatement, what the library refuses before it asks for a device,
and the designed case that shows what the corrected p-values are for."""
import ctypes as C

import numpy as np
import pytest

from frog_amd import _abi
from frog_amd.volume import fwe_p, glm_draw

import glm_restate as G

F4, F8 = np.float32, np.float64
# One f32 cast, 2^-24, on top of the f64 error of the normal equations: about cond(X)^2 x 2^-53 = 2 x 10^-10 at the design of
# condition 1.3 x 10^3 below, which the cast's half ulp swallows: 2^-23 relative to max(1, |value|) bounds both.
BAR = 2.0 ** -23


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F4 else a


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def close(got, want):
    got, want = np.asarray(got, F8), np.asarray(want, F8)
    return np.abs(got - want) / np.maximum(1.0, np.abs(want))


def test_the_two_forms_of_the_restatement_agree():
    rng = np.random.default_rng(5)
    for p, n in ((1, 6), (2, 9), (3, 12), (8, 14)):
        X = np.concatenate([np.ones((n, 1)), rng.normal(0, 1, (n, p - 1))], axis=1) if p > 1 else np.ones((n, 1))
        planes = rng.normal(0, 1, (n, 50)).astype(F4)
        planes[rng.random(planes.shape) < 0.3] = G.NAN
        planes[:, 3] = 2.5                                      # a constant value: an exact fit of the intercept
        region = (np.arange(50) % 7 != 0).astype(np.uint8)
        cons = np.concatenate([np.eye(p), -np.eye(p)])[:8]
        a = G.finish(planes, X, cons, 2, 0.0, region, -7.0)
        b = G.finish(planes, X, cons, 2, 0.0, region, -7.0, fitter=G.literal)
        assert all(same(u, v) for u, v in zip(a, b)), p
        assert a[4].any() and not a[4].all() and not a[4][::7].any()
        if p == 1:
            assert a[4][3] and a[1][3] == 0 and same(a[2][:, 3], np.full(2, G.NAN))      # t of an exact fit: the one NaN
        perm, sign = G.draw(n, 3, 11, True, True)
        Xp = G.design_rows(X, perm[2], sign[2], 1 if p == 1 else 2)
        va, vb = G.fit(planes, Xp, cons, 2), G.literal(planes, Xp, cons, 2)
        assert (va[0] == vb[0]).all() and va[0].any() and same(va[3][:, va[0]], vb[3][:, va[0]])
        assert not same(va[3][:, va[0]], G.fit(planes, X, cons, 2)[3][:, va[0]])          # the permutation moved the statistic


def test_restatement_against_lstsq_and_scipy():
    from scipy import stats
    rng = np.random.default_rng(17)
    n, V = 24, 40
    x = 18.6 + rng.uniform(0, 1, n)
    X = np.stack([np.ones(n), x], axis=1)
    assert 1.0e3 < np.linalg.cond(X) < 1.7e3
    Y = (rng.normal(0, 1, (n, V)) + 0.3 * x[:, None]).astype(F4)
    beta, sigma, t, count, fit = G.finish(Y, X, [[0.0, 1.0]])
    assert fit.all() and (count == n).all()
    want = np.linalg.lstsq(X, Y.astype(F8), rcond=None)[0]
    assert close(beta, want).max() <= BAR
    for v in range(V):
        r = stats.linregress(x, Y[:, v].astype(F8))
        assert close(t[0, v], r.slope / r.stderr) <= BAR and close(beta[1, v], r.slope) <= BAR and close(beta[0, v], r.intercept) <= BAR
    resid = Y.astype(F8) - X @ want
    assert close(sigma, np.sqrt((resid ** 2).sum(axis=0) / (n - 2))).max() <= BAR
    # two groups: the t of the group column is Student's two-sample t
    g = (np.arange(n) % 3 == 0).astype(F8)
    Xg = np.stack([np.ones(n), g], axis=1)
    tg = G.finish(Y, Xg, [[0.0, 1.0]])[2][0]
    want_t = stats.ttest_ind(Y[g == 1].astype(F8), Y[g == 0].astype(F8), axis=0).statistic
    assert close(tg, want_t).max() <= BAR
    # three columns with images left out per voxel: lstsq over the participating rows
    X3 = np.stack([np.ones(n), g, x - x.mean()], axis=1)
    Yh = Y.copy()
    Yh[rng.random(Yh.shape) < 0.2] = G.NAN
    b3, _, t3, k3, fit3 = G.finish(Yh, X3, [[0.0, 1.0, 0.0]])
    assert fit3.all() and k3.min() < n
    for v in range(V):
        S = ~np.isnan(Yh[:, v])
        bw, rss = np.linalg.lstsq(X3[S], Yh[S, v].astype(F8), rcond=None)[:2]
        cov = rss[0] / (S.sum() - 3) * np.linalg.inv(X3[S].T @ X3[S])
        assert close(b3[:, v], bw).max() <= BAR and close(t3[0, v], bw[1] / np.sqrt(cov[1, 1])) <= BAR


def test_draw_equals_its_restatement():
    lib = _abi.hip_lib()                                        # loads without a device
    for n, k, seed, shuffle, flip in ((20, 16, 0, True, False), (7, 9, 2 ** 63 + 5, True, True), (5, 4, 3, False, True), (1, 3, 1, True, True),
                                      (4096, 2, 9, True, True)):
        perm, sign = glm_draw(n, k, seed, shuffle, flip)
        want = G.draw(n, k, seed, shuffle, flip)
        assert same(perm, want[0]) and same(sign, want[1]), (n, seed)
        assert (perm[0] == np.arange(n)).all() and (sign[0] == 1).all()
        assert (np.sort(perm, axis=1) == np.arange(n)).all() and np.isin(sign, (-1, 1)).all()
        if shuffle and n > 4:
            assert (perm[1:] != np.arange(n)).any()
        if flip and n > 4:
            assert (sign[1:] == -1).any()
    buf, sg = (C.c_uint32 * 8)(), (C.c_int8 * 8)()
    assert lib.frog_glm_draw(4, 2, 0, 1, 0, buf, None) == _abi.FROG_OK          # no signs wanted
    for bad in ((0, 2, buf, sg), (4097, 2, buf, sg), (4, 0, buf, sg), (4, 2, None, sg)):
        assert lib.frog_glm_draw(bad[0], bad[1], 0, 1, 1, bad[2], bad[3]) == _abi.FROG_E_INVALID, bad[:2]
    assert lib.frog_glm_draw(4, 2, 0, 1, 1, buf, None) == _abi.FROG_E_INVALID   # flips without a place for them


def test_create_refuses_before_the_device_is_asked():
    """Each of these is FROG_E_INVALID also where there is no device, so none of them got as far as asking for one.  What
    needs a live accumulator (finish's and permute's arguments) is refused in tests/test_gpu_glm.py."""
    lib = _abi.hip_lib()
    grid = _abi.volume_view(None, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (5, 4, 3))
    h = C.c_void_p()
    X = np.ones((4097, 9))
    X[:, 1] = np.arange(4097)
    dp = X.ctypes.data_as(_abi.c_double_p)

    def create(n=6, p=2, first=0, planes=3, design=dp, g=C.byref(grid), out=C.byref(h)):
        return lib.frog_glm_create(g, first, planes, n, p, design, 0, out)

    for bad in (dict(g=None), dict(design=None), dict(out=None), dict(n=0), dict(n=4097), dict(p=0), dict(p=9), dict(n=2, p=2), dict(n=3, p=8),
                dict(first=3, planes=1), dict(first=1, planes=3), dict(planes=0)):
        assert create(**bad) == _abi.FROG_E_INVALID and not h.value, bad
    for value in (np.nan, np.inf, -np.inf):
        Xb = np.ones((6, 2))
        Xb[5, 1] = value
        assert create(design=Xb.ctypes.data_as(_abi.c_double_p)) == _abi.FROG_E_INVALID and not h.value
    planes = C.c_uint32()
    assert lib.frog_glm_planes(C.byref(grid), 4097, 0, C.byref(planes)) == _abi.FROG_E_INVALID
    assert lib.frog_glm_planes(None, 4, 0, C.byref(planes)) == _abi.FROG_E_INVALID
    # a NULL accumulator
    f = (C.c_float * 4)()
    con = (C.c_double * 2)(0.0, 1.0)
    assert lib.frog_glm_add(None, None, C.byref(grid), None, 1, 0.0) == _abi.FROG_E_INVALID
    assert lib.frog_glm_add_jacobian(None, None, None, None, 1) == _abi.FROG_E_INVALID
    assert lib.frog_glm_plane(None, 0, f) == _abi.FROG_E_INVALID
    assert lib.frog_glm_finish(None, 1, con, 1, 0.0, None, 0.0, f, f, f, None) == _abi.FROG_E_INVALID
    assert lib.frog_glm_permute(None, 1, con, 1, 0.0, None, 1, 1, (C.c_uint32 * 2)(), None, f, f) == _abi.FROG_E_INVALID
    lib.frog_glm_destroy(None)


DESIGNED_GRID = ((12, 10, 8), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
DESIGNED_PERMS, DESIGNED_SEED = 200, 4


def designed_case():
    """20 images of N(0, 1) noise (f32) on the 12 x 10 x 8 grid, 15 % of the entries dropped at random; the design is an
    intercept, an alternating group and a centred integer age; a 5 x 4 x 4 block holds +5 in group 1.  Returns (volumes,
    on-grid masks uint8, design, contrast of the group column, block bool)."""
    rng = np.random.default_rng(23)
    n, shape = 20, DESIGNED_GRID[0][::-1]
    group = np.arange(n) % 2
    age = rng.integers(20, 61, n).astype(F8)
    X = np.stack([np.ones(n), group.astype(F8), age - age.mean()], axis=1)
    vols = rng.normal(0, 1, (n,) + shape).astype(F4)
    block = np.zeros(shape, bool)
    block[2:6, 3:7, 4:9] = True
    vols[group == 1] += np.where(block, F4(5), F4(0))
    on = (rng.random((n,) + shape) >= 0.15).astype(np.uint8)
    return vols, on, X, np.array([[0.0, 1.0, 0.0]]), block


def designed_condition(p, t, fit, block):
    """Every block voxel has p < 0.05, at most 5 % of the others do; a vote on uncorrected t > 2 flags null voxels."""
    assert block.sum() == 80 and fit.all()
    assert (p[block] < 0.05).all()
    assert (p[~block] < 0.05).mean() <= 0.05
    assert (t[~block] > 2).any()


def test_designed_case_on_the_restatement():
    vols, on, X, con, block = designed_case()
    planes = np.where(on != 0, vols, G.NAN)
    _, _, t, count, fit = G.finish(planes, X, con)
    assert count.min() < 20 and count.min() >= 4
    perm, _ = G.draw(len(X), DESIGNED_PERMS, DESIGNED_SEED)
    hi, lo = G.permute(planes, X, con, perm, None, 2)
    assert same(hi[0], G.extrema(fit.reshape(-1), t.reshape(1, -1))[0])
    p = fwe_p(t[0], hi[:, 0], fit=fit)
    assert p.dtype == F4 and p.min() >= F4(1 / DESIGNED_PERMS) and p.max() <= 1
    designed_condition(p, t[0], fit, block)
    # the stated formula, voxel by voxel
    flat, pf = t[0].reshape(-1), p.reshape(-1)
    for v in range(0, flat.size, 37):
        assert pf[v] == F4((1 + int((hi[1:, 0] >= flat[v]).sum())) / F8(DESIGNED_PERMS))
    two = fwe_p(t[0], hi[:, 0], lo[:, 0], fit)
    # two-sided: the null maxima can only grow, so where t > 0 the p-value can only grow; still few null voxels beyond it
    assert (two[t[0] > 0] >= p[t[0] > 0]).all() and (two[~block] < 0.05).mean() <= 0.05
    assert fwe_p(np.array([np.nan, 100.0, -100.0], F4), hi[:, 0]).tolist() == [1.0, F4(1 / F8(DESIGNED_PERMS)), 1.0]      # NaN; beyond every maximum; below
