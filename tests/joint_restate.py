"""frog_jlabels (include/frog_chain.h) restated in NumPy from the header's text: joint label fusion of atlases that are
already on the target's grid.  Every line of the header is one NumPy operation in float64, vectorised over the voxels; the
loops over the patch taps (z, then y, then x), over the pairs and over the indices of the LDL^T run in the stated order, so
the tests compare with ==.

The active set differs from voxel to voxel.  The vectorised solve keeps all N rows and forces L_ij = +0.0 where atlas i or j
is not active, D_j = 1, z_j = y_j = w_j = +0.0 where j is not: every term such a row contributes to an active one is
(+0.0 * +0.0) * 1 = +0.0 or +0.0 * +0.0, and x - (+0.0) is x for every x, so the active rows carry the bits of the system
restricted to them.  solve_literal is that restricted system for one voxel in Python floats; test_jlabels.py holds the two
against each other."""
import numpy as np

from wlabels_restate import probability, staged            # the same staging and the same score / total

__all__ = ["staged", "probability", "patch_stats", "gram", "solve", "solve_literal", "weights", "restate"]


def _taps(r):
    return [(dz, dy, dx) for dz in range(2 * r + 1) for dy in range(2 * r + 1) for dx in range(2 * r + 1)]


def _window(shape, tap):
    return tuple(slice(o, o + n) for o, n in zip(tap, shape))


def patch_stats(x, valid, radius):
    """(mean, inv) of X over the patch voxels where X is valid."""
    r = int(radius)
    X = np.pad(np.where(valid, x, np.float32(0)).astype(np.float64), r)
    V = np.pad(valid, r)
    n, s, ss = (np.zeros(x.shape, np.float64) for _ in range(3))
    for tap in _taps(r):
        w = _window(x.shape, tap)
        xu = X[w]
        n = np.where(V[w], n + 1.0, n)
        s = np.where(V[w], s + xu, s)
        ss = np.where(V[w], ss + xu * xu, ss)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        var = (n * ss - s * s) / (n * n)
        mean = s / n
        inv = np.where((n >= 2) & (var > 0), 1.0 / np.sqrt(var), 0.0)
    return mean, inv


def gram(t, valid_t, images, radius):
    """M[i][j] (j <= i) of the differences of the patch-normalised atlases from the patch-normalised target."""
    r = int(radius)
    shape = t.shape
    pad = lambda x, v: (np.pad(np.where(v, x, np.float32(0)).astype(np.float64), r), np.pad(v, r))
    T, VT = pad(t, valid_t)
    mean_t, inv_t = patch_stats(t, valid_t, r)
    A = [pad(a, v) for a, v in images]
    stats = [patch_stats(a, v, r) for a, v in images]
    n = len(images)
    M = [[np.zeros(shape, np.float64) for _ in range(i + 1)] for i in range(n)]
    for tap in _taps(r):
        w = _window(shape, tap)
        with np.errstate(invalid="ignore", over="ignore"):
            th = (T[w] - mean_t) * inv_t
            d = []
            for (Ai, Vi), (mean, inv) in zip(A, stats):
                ah = (Ai[w] - mean) * inv
                d.append(np.where(VT[w] & Vi[w], np.fabs(ah - th), 0.0))
            for i in range(n):
                for j in range(i + 1):
                    p = d[i] * d[j]
                    M[i][j] = M[i][j] + p
    return M


def solve(K, active):
    """K w = 1 by the header's LDL^T on the rows of `active` (bool per atlas and voxel); returns (raw w, normalised w)."""
    n = len(K)
    shape = K[0][0].shape
    zero, one = np.zeros(shape, np.float64), np.ones(shape, np.float64)
    L = [[None] * n for _ in range(n)]
    D = [None] * n
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for j in range(n):
            dj = K[j][j]
            for k in range(j):
                q = L[j][k] * L[j][k]
                dj = dj - q * D[k]
            D[j] = np.where(active[j], dj, one)
            for i in range(j + 1, n):
                x = K[i][j]
                for k in range(j):
                    q = L[i][k] * L[j][k]
                    x = x - q * D[k]
                L[i][j] = np.where(active[i] & active[j], x / D[j], zero)
        z = [None] * n
        for i in range(n):
            zi = one
            for k in range(i):
                zi = zi - L[i][k] * z[k]
            z[i] = np.where(active[i], zi, zero)
        y = [np.where(active[i], z[i] / D[i], zero) for i in range(n)]
        w = [None] * n
        for i in range(n - 1, -1, -1):
            wi = y[i]
            for k in range(i + 1, n):
                wi = wi - L[k][i] * w[k]
            w[i] = np.where(active[i], wi, zero)
        S = zero
        for i in range(n):
            S = np.where(active[i], S + w[i], S)
        norm = [np.where(active[i], w[i] / S, zero) for i in range(n)]
    return w, norm


def solve_literal(K):
    """The header's solve for one voxel: K a list of rows of Python floats (the active atlases only).  (raw, normalised)."""
    n = len(K)
    L = [[0.0] * n for _ in range(n)]
    D = [0.0] * n
    for j in range(n):
        D[j] = K[j][j]
        for k in range(j):
            q = L[j][k] * L[j][k]
            D[j] = D[j] - q * D[k]
        for i in range(j + 1, n):
            x = K[i][j]
            for k in range(j):
                q = L[i][k] * L[j][k]
                x = x - q * D[k]
            L[i][j] = x / D[j]
    z = [0.0] * n
    for i in range(n):
        z[i] = 1.0
        for k in range(i):
            z[i] = z[i] - L[i][k] * z[k]
    y = [z[i] / D[i] for i in range(n)]
    w = [0.0] * n
    for i in range(n - 1, -1, -1):
        w[i] = y[i]
        for k in range(i + 1, n):
            w[i] = w[i] - L[k][i] * w[k]
    S = 0.0
    for i in range(n):
        S = S + w[i]
    return w, [wi / S for wi in w]


def weights(t, valid_t, images, radius, beta, alpha):
    """images: [(a, valid_a)] in call order.  Returns a dict: K (lower triangle, [i][j]), active [i], raw and norm (float64
    per atlas: before and after the division by S; +0.0 where the atlas is not active), w (float32)."""
    M = gram(t, valid_t, images, radius)
    n = len(images)
    K = [[None] * (i + 1) for i in range(n)]
    for i in range(n):
        for j in range(i + 1):
            k = M[i][j]
            for _ in range(int(beta) - 1):
                k = k * M[i][j]
            K[i][j] = k
        K[i][i] = K[i][i] + np.float64(alpha)
    active = [valid_t & v for _, v in images]
    raw, norm = solve(K, active)
    with np.errstate(over="ignore", invalid="ignore"):
        w = [x.astype(np.float32) for x in norm]
    return {"K": K, "active": active, "raw": raw, "norm": norm, "w": w}


def restate(target, atlases, radius, beta, alpha, fill_label=0, target_inside=None):
    """target: array on the grid; atlases: (image, labels) or (image, labels, inside) per atlas in call order, all on the
    grid.  Returns what wlabels_restate.restate returns, and weights[i] (float32; 0 where atlas i is not active)."""
    t, valid_t = staged(target, target_inside)
    images = [staged(at[0], at[2] if len(at) > 2 else None) for at in atlases]
    label_maps = [np.asarray(at[1]).astype(np.int64) for at in atlases]
    values = np.unique(np.concatenate([l.ravel() for l in label_maps]))
    jw = weights(t, valid_t, images, radius, beta, alpha)
    scores = np.zeros((len(values),) + t.shape, np.float32)
    for lab, w, active in zip(label_maps, jw["w"], jw["active"]):
        idx = np.searchsorted(values, lab)
        for l in range(len(values)):
            hit = active & (idx == l)
            with np.errstate(invalid="ignore", over="ignore"):
                scores[l] = np.where(hit, scores[l] + w, scores[l])
    total = np.zeros(t.shape, np.float32)
    best = np.zeros(t.shape, np.float32)
    winner = np.zeros(t.shape, np.int64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for l in range(len(values)):
            total = total + scores[l]
            better = scores[l] > best                               # strictly larger than every earlier one, and > 0
            best = np.where(better, scores[l], best)
            winner = np.where(better, l, winner)
        some = total != 0
        confidence = np.where(some, best / total, np.float32(0)).astype(np.float32)
    return {"values": values, "scores": scores, "total": total, "labels": np.where(some, values[winner], np.int64(fill_label)),
            "confidence": confidence, "weights": jw["w"], "active": jw["active"]}
