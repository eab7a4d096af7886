"""frog_staple (include/frog_chain.h) restated in NumPy, line by line: multi-label STAPLE (Warfield, Zou, Wells, IEEE TMI
23(7), 2004) with u64 sums and one separately rounded f64 operation per stated line.  No log or exp: np.frexp, np.ldexp and
np.rint give the bits the device gives, so the tests compare with ==."""
import numpy as np

FLOOR = 2.0 ** -24
ONE = 1 << 30
K = 16


def dense(volumes):
    """(values, idx): the sorted distinct label values (int64) and one flat index array per volume (the position of each
    voxel's value in `values`).  A volume object that appears more than once is indexed once."""
    vols = [np.asarray(v) for v in volumes]
    values = np.unique(np.concatenate([np.unique(v).astype(np.int64) for v in {id(v): v for v in vols}.values()]))
    cache = {}
    idx = []
    for v in vols:
        if id(v) not in cache:
            cache[id(v)] = np.searchsorted(values, v.astype(np.int64).ravel()).astype(np.int16)
        idx.append(cache[id(v)])
    return values, idx


def start_theta(n, L, p0):
    """theta[i][l'][l] = P(image i shows l' | truth l): p0 on the diagonal, (1 - p0) / (L - 1) elsewhere."""
    theta = np.empty((n, L, L), np.float64)
    if L > 1:
        theta[:] = (1.0 - np.float64(p0)) / np.float64(L - 1)
    theta[:, np.arange(L), np.arange(L)] = np.float64(p0)
    return theta


def e_step(Da, theta, prior, renormalise=True):
    """q[v][l] (uint32, A x L) of the active voxels whose dense labels are Da[i][v].  renormalise=False leaves the frexp
    steps out: the plain f64 product, which underflows for large groups (the tests show it)."""
    n, A = Da.shape
    L = len(prior)
    m = np.repeat(prior[None, :], A, 0)
    e = np.zeros((A, L), np.int64)
    for i in range(n):
        m = m * np.maximum(theta[i][Da[i]], FLOOR)
        if renormalise and (i % K == K - 1 or i == n - 1):
            m, k = np.frexp(m)
            e += k
    if not renormalise:
        return m
    emax = np.where(m > 0, e, np.iinfo(np.int64).min).max(1)
    p = np.ldexp(m, (e - emax[:, None]).clip(-100000, 0).astype(np.int32))
    s = np.zeros(A, np.float64)
    for l in range(L):
        s = s + p[:, l]
    return np.rint((p / s[:, None]) * np.float64(ONE)).astype(np.uint32)


def m_step(Da, q, theta):
    """(theta_new, S, T, change): u64 sums, then one f64 division per entry; the previous value where T[l] == 0."""
    n, A = Da.shape
    L = q.shape[1]
    q64 = q.astype(np.uint64)
    T = q64.sum(0, dtype=np.uint64)
    S = np.zeros((n, L, L), np.uint64)
    order = {}
    for i in range(n):
        key = Da[i].tobytes() if A < 4096 else None
        if key is not None and key in order:
            S[i] = S[order[key]]
            continue
        for lp in np.unique(Da[i]):
            S[i, lp] = q64[Da[i] == lp].sum(0, dtype=np.uint64)
        if key is not None:
            order[key] = i
    new = theta.copy()
    ok = T > 0
    new[:, :, ok] = S[:, :, ok].astype(np.float64) / T[ok].astype(np.float64)
    change = float(np.abs(new - theta).max())
    return new, S, T, change


def restate(volumes, p0=0.99, tol=1e-6, max_iter=50, restrict=False):
    """Every output of frog_staple_solve and its getters as a dict: values, q (uint32, L x voxels, flat x fastest), labels
    (int64), confidence (float32), theta, sums, totals, prior, iterations, change, active_voxels."""
    values, idx = dense(volumes)
    n, L, V = len(idx), len(values), len(idx[0])
    distinct = list({id(d): d for d in idx}.values())       # a volume given more than once is looked at once
    unanimous = np.ones(V, bool)
    for d in distinct[1:]:
        unanimous &= d == distinct[0]
    active = ~unanimous if restrict else np.ones(V, bool)
    A = int(active.sum())
    gathered = {id(d): d[active].astype(np.int64) for d in distinct}
    Da = np.stack([gathered[id(d)] for d in idx])
    q = np.zeros((V, L), np.uint32)
    q[~active, idx[0][~active]] = ONE
    theta = start_theta(n, L, p0)
    S, T = np.zeros((n, L, L), np.uint64), np.zeros(L, np.uint64)
    prior = np.zeros(L, np.float64)
    it, change = 0, float("inf")
    if A:
        c = np.bincount(Da.ravel(), minlength=L).astype(np.uint64)
        prior = c.astype(np.float64) / np.float64(n * A)
        while True:
            qa = e_step(Da, theta, prior)
            if it == max_iter:
                break
            theta, S, T, change = m_step(Da, qa, theta)
            it += 1
            if change < tol:
                qa = e_step(Da, theta, prior)
                break
        q[active] = qa
    winner = np.argmax(q, axis=1)                   # the first of the largest: the smallest value of a tie
    best = q[np.arange(V), winner]
    return {
        "values": values, "q": np.ascontiguousarray(q.T), "labels": values[winner],
        "confidence": (best.astype(np.float64) * 2.0 ** -30).astype(np.float32),
        "theta": theta, "sums": S, "totals": T, "prior": prior, "iterations": it, "change": change, "active_voxels": A,
    }


def probability(r, value):
    """float32 of (double)q * 2^-30 for one label value, flat."""
    l = int(np.searchsorted(r["values"], value))
    assert r["values"][l] == value
    return (r["q"][l].astype(np.float64) * 2.0 ** -30).astype(np.float32)


def sensitivity(r):
    """theta[i][l][l]: (n, L)."""
    L = len(r["values"])
    return r["theta"][:, np.arange(L), np.arange(L)]


def designed_group(shape=(7, 13, 19), error=0.3, seed=5):
    """(truth, volumes, R): three boxes (labels 1, 2, 3) on background 0; images 0-1 equal truth, images 2-4 each replace
    `error` of the voxels by a different label, and all three carry label 2 in the 1 x 3 x 3 region R inside label 1."""
    rng = np.random.default_rng(seed)
    truth = np.zeros(shape, np.int16)
    truth[1:5, 2:9, 2:9] = 1
    truth[2:6, 4:11, 11:17] = 2
    truth[0:3, 9:13, 3:9] = 3
    R = np.zeros(shape, bool)
    R[3, 4:7, 4:7] = True
    assert (truth[R] == 1).all() and R.sum() == 9
    vols = [truth.copy(), truth.copy()]
    for _ in range(3):
        v = truth.copy()
        flip = rng.random(shape) < error
        v[flip] = (truth[flip] + rng.integers(1, 4, int(flip.sum()))) % 4
        v[R] = 2
        vols.append(v)
    return truth, vols, R


def noisy_group(n, error, L=4, shape=(7, 13, 19), seed=7, values=None, cyclic=False):
    """(truth, volumes): a blocky truth with L labels and n images that each replace a share of the voxels by a different
    label (cyclic: by the next one, so that an image never shows the others for it and their theta falls to 0); `error` is
    one rate or one per image.  `values` maps the dense labels to label values."""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    truth = ((x // 3) + 2 * (y // 4) + 3 * (z // 2)) % L
    rates = np.broadcast_to(np.asarray(error, np.float64), (n,))
    vols = []
    for i in range(n):
        v = truth.copy()
        if L > 1:
            flip = rng.random(shape) < rates[i]
            v[flip] = (truth[flip] + (1 if cyclic else rng.integers(1, L, int(flip.sum())))) % L
        vols.append(v)
    if values is not None:
        values = np.asarray(values)
        truth, vols = values[truth], [values[v] for v in vols]
    return truth, vols
