"""frog_glm (include/frog_chain.h) restated: the stored planes come from cover_restate.terms (value and validity, as
frog_rank's do), then the model, one float64 operation per line as the header states them, in two forms that must agree with
==: `literal`, a loop over the voxels and over each voxel's participating images alone, and the vectorised functions, where
an image that does not take part adds +0.0 (the device's trick).  frog_glm_draw's generator is restated in Python integers."""
import numpy as np

import cover_restate
import rank_restate

F4, F8, U4 = np.float32, np.float64, np.uint32
NAN = U4(0x7FC00000).view(F4)
M64 = (1 << 64) - 1


def entries(x, valid):
    """What an add keeps: x where the voxel is valid and x is finite, 0x7FC00000 elsewhere."""
    return np.where(valid & np.isfinite(x), x.astype(F4), NAN)


def collect(images, grid, interpolation=1, background=0.0, reslicer=cover_restate.reslice):
    """`images` as cover_restate.restate takes them: the (N,) + shape stored planes."""
    return np.stack([entries(*cover_restate.terms(links, volume, origin, spacing, grid, mask, interpolation, background, reslicer)[:2])
                     for links, volume, origin, spacing, mask in images])


def splitmix(seed):
    s = int(seed) & M64
    while True:
        s = (s + 0x9E3779B97F4A7C15) & M64
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        yield z ^ (z >> 31)


def draw(n, n_perms, seed=0, shuffle=True, flip=False):
    """(perm uint32, sign int8), both (n_perms, n)."""
    g = splitmix(seed)
    perm, sign = np.empty((n_perms, n), U4), np.ones((n_perms, n), np.int8)
    for k in range(n_perms):
        row = list(range(n))
        if k and shuffle:
            for i in range(n - 1, 0, -1):
                j = next(g) % (i + 1)
                row[i], row[j] = row[j], row[i]
        perm[k] = row
        if k and flip:
            for i in range(n):
                sign[k, i] = -1 if next(g) >> 63 else 1
    return perm, sign


def design_rows(X, perm=None, sign=None, columns=0):
    """X' of one permutation: the columns whose bit is set hold sign[i] * X[perm[i]][j], one multiplication."""
    X = np.asarray(X, F8)
    Xp = X.copy()
    if perm is None:
        return Xp
    s = np.ones(len(X), F8) if sign is None else np.asarray(sign).astype(F8)
    for j in range(X.shape[1]):
        if (int(columns) >> j) & 1:
            Xp[:, j] = s * X[np.asarray(perm), j]
    return Xp


def _solve(L, D, rhs):
    """forward, diagonal, backward with the factor; rhs: p values (scalars or arrays), returned new."""
    p = len(D)
    z = list(rhs)
    for i in range(p):
        for q in range(i):
            m = L[i][q] * z[q]
            z[i] = z[i] - m
    for i in range(p):
        z[i] = z[i] / D[i]
    for i in range(p - 1, -1, -1):
        for q in range(i + 1, p):
            m = L[q][i] * z[q]
            z[i] = z[i] - m
    return z


def _factor(A):
    """LDL^T of the lower triangle A[r][c] (c <= r), frog_jlabels_finish's loops; (L, D, ok)."""
    p = len(A)
    L = [[None] * p for _ in range(p)]
    D = [None] * p
    ok = True
    for j in range(p):
        dj = A[j][j]
        for q in range(j):
            sq = L[j][q] * L[j][q]
            m = sq * D[q]
            dj = dj - m
        D[j] = dj
        limit = F8(2.0 ** -40) * A[j][j]
        ok = ok & (A[j][j] > 0) & (dj > limit)
        for i in range(j + 1, p):
            x = A[i][j]
            for q in range(j):
                lq = L[i][q] * L[j][q]
                m = lq * D[q]
                x = x - m
            L[i][j] = x / dj
    return L, D, ok


def _contrast(L, D, beta, s2, sd, con, sigma_floor):
    p = len(D)
    u = _solve(L, D, [np.full(np.shape(s2), con[j], F8) for j in range(p)])
    v = np.zeros(np.shape(s2), F8)
    e = np.zeros(np.shape(s2), F8)
    for j in range(p):
        m = F8(con[j]) * u[j]
        v = v + m
    for j in range(p):
        m = F8(con[j]) * beta[j]
        e = e + m
    den = s2 * v
    den = np.sqrt(den)
    g = e / den
    t = np.asarray(g, F8).astype(F4)
    return np.where((sd <= sigma_floor) | ~np.isfinite(t), NAN, t)


def fit(planes, Xp, contrasts, min_count=1, sigma_floor=0.0, region=None):
    """Vectorised.  planes (n, V) float32 stored values, Xp (n, p) the design rows as used.  Returns (fit bool (V,), beta
    (p, V) float64, sd (V,) float64, t (C, V) float32 with the canonical NaN, k (V,))."""
    planes = np.asarray(planes, F4)
    n, V = planes.shape
    p = Xp.shape[1]
    take = ~np.isnan(planes)
    y = np.where(take, planes, F4(0)).astype(F8)
    k = take.sum(axis=0)
    wanted = k >= max(min_count, p + 1)
    if region is not None:
        wanted &= np.asarray(region).reshape(-1) != 0
    zero = np.zeros(V, F8)
    with np.errstate(all="ignore"):
        A = [[zero.copy() for _ in range(r + 1)] for r in range(p)]
        b = [zero.copy() for _ in range(p)]
        for i in range(n):
            for r in range(p):
                for c in range(r + 1):
                    m = Xp[i, r] * Xp[i, c]
                    A[r][c] = A[r][c] + np.where(take[i], m, F8(0))
            for r in range(p):
                m = Xp[i, r] * y[i]
                b[r] = b[r] + m
        L, D, ok = _factor(A)
        beta = _solve(L, D, b)
        rss = zero.copy()
        for i in range(n):
            f = zero.copy()
            for j in range(p):
                m = Xp[i, j] * beta[j]
                f = f + m
            r = y[i] - f
            q = r * r
            rss = rss + np.where(take[i], q, F8(0))
        s2 = rss / np.maximum(k - p, 1).astype(F8)
        sd = np.sqrt(s2)
        t = [_contrast(L, D, beta, s2, sd, con, sigma_floor) for con in np.asarray(contrasts, F8).reshape(-1, p)]
    assert all(v.dtype == F8 for v in beta) and sd.dtype == F8
    return wanted & ok, np.stack(beta), sd, np.stack(t).astype(F4) if t else np.empty((0, V), F4), k


def literal(planes, Xp, contrasts, min_count=1, sigma_floor=0.0, region=None):
    """The same, voxel by voxel over the participating images only, in float64 scalars."""
    planes = np.asarray(planes, F4)
    n, V = planes.shape
    p = Xp.shape[1]
    cons = np.asarray(contrasts, F8).reshape(-1, p)
    fitv, beta, sd, t, kk = np.zeros(V, bool), np.zeros((p, V), F8), np.zeros(V, F8), np.full((len(cons), V), NAN, F4), np.zeros(V, np.int64)
    with np.errstate(all="ignore"):
        for v in range(V):
            S = [i for i in range(n) if not np.isnan(planes[i, v])]
            k = kk[v] = len(S)
            if k < max(min_count, p + 1) or (region is not None and not np.asarray(region).reshape(-1)[v]):
                continue
            A = [[F8(0)] * (r + 1) for r in range(p)]
            b = [F8(0)] * p
            for i in S:
                for r in range(p):
                    for c in range(r + 1):
                        m = Xp[i, r] * Xp[i, c]
                        A[r][c] = A[r][c] + m
                y = F8(planes[i, v])
                for r in range(p):
                    m = Xp[i, r] * y
                    b[r] = b[r] + m
            L, D, ok = _factor(A)
            bt = _solve(L, D, b)
            rss = F8(0)
            for i in S:
                f = F8(0)
                for j in range(p):
                    m = Xp[i, j] * bt[j]
                    f = f + m
                r = F8(planes[i, v]) - f
                q = r * r
                rss = rss + q
            s2 = rss / F8(k - p)
            s = np.sqrt(s2)
            fitv[v], beta[:, v], sd[v] = bool(ok), bt, s
            for ci, con in enumerate(cons):
                t[ci, v] = _contrast(L, D, bt, s2, s, con, sigma_floor)
    return fitv, beta, sd, t, kk


def finish(planes, X, contrasts, min_count=1, sigma_floor=0.0, region=None, fill=0.0, fitter=fit):
    """frog_glm_finish on planes (n,) + shape: (beta float32 (p,) + shape, sigma float32, t float32 (C,) + shape, count uint16,
    fit bool)."""
    planes = np.asarray(planes, F4)
    shape = planes.shape[1:]
    X = np.asarray(X, F8)
    ok, beta, sd, t, k = fitter(planes.reshape(len(planes), -1), design_rows(X), contrasts, min_count, sigma_floor, region)
    with np.errstate(all="ignore"):
        b = np.where(ok, beta.astype(F4), F4(fill))
        s = np.where(ok, sd.astype(F4), F4(fill))
    t = np.where(ok, t, F4(fill))
    return (b.reshape((-1,) + shape), s.reshape(shape), t.astype(F4).reshape((-1,) + shape), k.astype(np.uint16).reshape(shape),
            ok.reshape(shape))


def extrema(ok, t):
    """(max, min) per contrast over the fit voxels whose t is not NaN, in the order of frog_rank's keys; -inf and +inf where
    there is none."""
    hi, lo = np.full(len(t), -np.inf, F4), np.full(len(t), np.inf, F4)
    for c in range(len(t)):
        vals = t[c][ok & ~np.isnan(t[c])]
        if len(vals):
            keys = rank_restate.keys_of(vals)
            hi[c], lo[c] = rank_restate.values_of(keys.max()[None])[0], rank_restate.values_of(keys.min()[None])[0]
    return hi, lo


def permute(planes, X, contrasts, perm, sign=None, columns=None, min_count=1, sigma_floor=0.0, region=None):
    """frog_glm_permute: (max_t, min_t), float32 (n_perms, C)."""
    planes = np.asarray(planes, F4)
    X = np.asarray(X, F8)
    bits = (1 << X.shape[1]) - 1 if columns is None else columns
    flat = planes.reshape(len(planes), -1)
    out = [extrema(*(lambda r: (r[0], r[3]))(fit(flat, design_rows(X, perm[k], None if sign is None else sign[k], bits), contrasts,
                                                   min_count, sigma_floor, region))) for k in range(len(perm))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
