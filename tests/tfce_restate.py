"""Threshold-free cluster enhancement (frog_tfce and frog_tfce_volume, include/frog_chain.h) restated in NumPy, line by line:
the level of a statistic by one f64 division and a truncation, the components of every level's mask by
clusters_restate.components, and per voxel the f64 sum of g(extent) * w_k over its levels in descending order."""
import numpy as np

import clusters_restate as R

F4, F8 = np.float32, np.float64


def levels(t, dh, side=0):
    """uint8: trunc((double)s / (double)dh) saturated at 255, s = t (side 0) or -t (side 1); 0 where t is NaN or s <= 0."""
    t = np.asarray(t, F4)
    s = -t if side else t
    ok = s > 0                                              # False for the NaN
    with np.errstate(over="ignore", invalid="ignore"):
        q = np.where(ok, s, F4(0)).astype(F8) / F8(F4(dh))
    return np.where(ok, np.where(q >= 255.0, 255.0, np.floor(q)), 0.0).astype(np.uint8)


def weights(dh, h):
    """w_k for k = 0..255 (w_0 is not used): (h == 2 ? h_k * h_k : h_k) * dh with h_k = k * dh, f64 products of the f32 dh."""
    d = F8(F4(dh))
    hk = np.arange(256, dtype=F8) * d
    return (hk * hk if h == 2 else hk) * d


def level_extents(level, connectivity=26):
    """[(k, M_k, e_k)] for k from the highest level down to 1: the mask level >= k and, on it, the extent of each voxel's
    component as f64 (anything elsewhere).  What every choice of dh, e and h shares."""
    level = np.asarray(level, np.uint8)
    out = []
    for k in range(int(level.max(initial=0)), 0, -1):       # descending: part of the statement
        mask = level >= k
        labels, n, _ = R.components(mask, connectivity)
        out.append((k, mask, np.bincount(labels.reshape(-1), minlength=n + 1).astype(F8)[labels]))
    return out


def enhance(level, dh, e=0.5, h=2, connectivity=26, extents=None):
    """float32 on the grid: the enhancement of a uint8 level map (extents: level_extents of it, where the caller has them)."""
    assert e in (0.5, 1) and h in (1, 2)
    w = weights(dh, h)
    acc = np.zeros(np.shape(level), F8)
    for k, mask, extent in level_extents(level, connectivity) if extents is None else extents:
        g = np.sqrt(extent) if e == 0.5 else extent
        m = g * w[k]
        acc = np.where(mask, acc + m, acc)
    with np.errstate(over="ignore"):
        return acc.astype(F4)


def tfce(t, dh=0.1, e=0.5, h=2, connectivity=26, side=0):
    """(tfce float32, its maximum): what frog_tfce_volume gives for the float32 array t[z, y, x]."""
    out = enhance(levels(t, dh, side), dh, e, h, connectivity)
    return out, out.max(initial=F4(0))


def tfce_p(tfce, null):
    """(float32)((1 + #{k >= 1: null[k] >= |tfce|}) / (double)n_perms), 1 where tfce == 0: counted one voxel at a time."""
    t = np.abs(np.asarray(tfce, F4))
    null = np.asarray(null, F4)
    out = np.empty(t.shape, F4)
    for i, v in np.ndenumerate(t):
        out[i] = F4(1) if v == 0 else F4((1 + int((null[1:] >= v).sum())) / F8(len(null)))
    return out
