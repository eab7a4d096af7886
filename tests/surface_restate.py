"""The surface distances of include/frog_chain.h (frog_distance_map, frog_surface) restated in NumPy: brute force over whole
lines by broadcasting, every line one rounded float64 operation or an integer operation, so the tests compare with ==.  And a
second, independent brute force over all feature voxels in 3-D."""
import numpy as np

ROW = np.dtype([("n_a", np.uint64), ("n_b", np.uint64), ("sum_ab", np.uint64), ("sum_ba", np.uint64),
                ("max_ab", np.uint32), ("max_ba", np.uint32), ("pct_ab", np.uint32), ("pct_ba", np.uint32)])
NONE = 0xFFFFFFFF


def surface(m, value):
    """The surface voxels of {m == value}: in the set, with a face neighbour that is not (outside the grid counts)."""
    a = np.asarray(m) == value
    p = np.pad(a, 1, constant_values=False)
    inside = (p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1] & p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:])
    return a & ~inside


def _weights(n, s):
    k = np.arange(n)
    d = (k[:, None] - k[None, :]).astype(np.float64) * np.float64(s)        # [p, q]: (double)(p - q) * s
    return d * d


def _along(g, axis, s):
    """min over q of ( g[.., q, ..] + ((double)(p - q) * s)^2 ) along `axis`."""
    g = np.moveaxis(g, axis, -1)
    out = (g[..., None, :] + _weights(g.shape[-1], s)).min(-1)
    return np.moveaxis(out, -1, axis)


def squared_distance(features, spacing):
    """g3 of the boolean array features[z, y, x] at spacing (sx, sy, sz)."""
    f = np.asarray(features, bool)
    sx, sy, sz = spacing
    g1 = np.where(f[..., None, :], _weights(f.shape[2], sx), np.inf).min(-1)
    return _along(_along(g1, 1, sy), 0, sz)


def brute_force_squared_distance(features, spacing):
    """Per voxel the minimum over all feature voxels of ((dx sx)^2 + (dy sy)^2) + (dz sz)^2."""
    f = np.asarray(features, bool)
    sx, sy, sz = (np.float64(s) for s in spacing)
    fz, fy, fx = np.nonzero(f)
    if not len(fx):
        return np.full(f.shape, np.inf)
    z, y, x = (c.ravel() for c in np.indices(f.shape))
    dx = (x[:, None] - fx[None, :]).astype(np.float64) * sx
    dy = (y[:, None] - fy[None, :]).astype(np.float64) * sy
    dz = (z[:, None] - fz[None, :]).astype(np.float64) * sz
    return ((dx * dx + dy * dy) + dz * dz).min(1).reshape(f.shape)


def fixed(g):
    """The stored distance: uint32 in units of 2^-16, 0xFFFFFFFF for +inf, at most 0xFFFFFFFE otherwise."""
    g = np.asarray(g, np.float64)
    u = np.minimum(np.rint(np.sqrt(g) * 65536.0), 4294967294.0)
    return np.where(np.isinf(g), 4294967295.0, u).astype(np.uint32)


def distance_map(m, value, spacing, mode):
    f = surface(m, value) if mode else np.asarray(m) == value
    return fixed(squared_distance(f, spacing))


def kth(n, p):
    """The 1-based rank of percentile p among n distances."""
    return (p * n + 99) // 100


def rows(image, reference, values, spacing, percentile=95):
    """One ROW per value: the image's label map against the reference's."""
    out = np.zeros(len(values), ROW)
    for r, value in zip(out, values):
        sa, sb = surface(image, value), surface(reference, value)
        r["n_a"], r["n_b"] = int(sa.sum()), int(sb.sum())
        r["max_ab"] = r["max_ba"] = r["pct_ab"] = r["pct_ba"] = NONE
        if not r["n_a"] or not r["n_b"]:
            continue
        ab = np.sort(fixed(squared_distance(sb, spacing))[sa])
        ba = np.sort(fixed(squared_distance(sa, spacing))[sb])
        r["sum_ab"], r["sum_ba"] = ab.sum(dtype=np.uint64), ba.sum(dtype=np.uint64)
        r["max_ab"], r["max_ba"] = ab[-1], ba[-1]
        r["pct_ab"], r["pct_ba"] = ab[kth(len(ab), percentile) - 1], ba[kth(len(ba), percentile) - 1]
    return out


def metrics(r):
    """(hausdorff, hausdorff_p, assd) of ROWs in float64, NaN where a surface is empty."""
    r = np.atleast_1d(r)
    n = len(r)
    h, hp, assd = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
    for k, x in enumerate(r):
        if int(x["n_a"]) and int(x["n_b"]):
            h[k] = float(max(int(x["max_ab"]), int(x["max_ba"]))) * 2.0 ** -16
            hp[k] = float(max(int(x["pct_ab"]), int(x["pct_ba"]))) * 2.0 ** -16
            assd[k] = (float(int(x["sum_ab"]) + int(x["sum_ba"])) / float(int(x["n_a"]) + int(x["n_b"]))) * 2.0 ** -16
    return h, hp, assd
