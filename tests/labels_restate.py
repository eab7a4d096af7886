"""frog_labels (include/frog_chain.h) restated in NumPy: the vote counts of N label arrays on one grid and everything the
library derives from them.  Integer arithmetic and one float32 division: the tests compare with ==."""
import numpy as np


def restate(volumes):
    """values: the sorted distinct label values (int64); counts[l]: how many arrays carry values[l], per voxel;
    labels: the value with the largest count, ties to the smallest value (int64); agreement: float32(c) / float32(N) of
    that count; voxels[l] = sum c, pairs[l] = sum c (c - 1) / 2 (uint64)."""
    vols = [np.asarray(v).astype(np.int64) for v in volumes]
    n = len(vols)
    values = np.unique(np.concatenate([v.ravel() for v in vols]))
    counts = np.zeros((len(values),) + vols[0].shape, np.int32)
    for v in vols:
        idx = np.searchsorted(values, v)
        np.add.at(counts, (idx,) + tuple(np.indices(v.shape)), 1)
    winner = np.argmax(counts, axis=0)              # the first maximum along ascending values: the smallest value of a tie
    best = np.take_along_axis(counts, winner[None], 0)[0]
    return {
        "n": n,
        "values": values,
        "counts": counts,
        "labels": values[winner],
        "agreement": best.astype(np.float32) / np.float32(n),
        "voxels": counts.reshape(len(values), -1).sum(1, dtype=np.int64).astype(np.uint64),
        "pairs": (counts * (counts - 1) // 2).reshape(len(values), -1).sum(1, dtype=np.int64).astype(np.uint64),
    }


def probability(r, value):
    """float32(c_value) / float32(N) per voxel."""
    l = int(np.searchsorted(r["values"], value))
    assert r["values"][l] == value
    return r["counts"][l].astype(np.float32) / np.float32(r["n"])


def dice(r):
    """2 pairs / ((N - 1) voxels) in float64: the pooled pairwise Dice overlap per label."""
    return 2.0 * r["pairs"].astype(np.float64) / ((r["n"] - 1.0) * r["voxels"].astype(np.float64))


def brute_force_dice(volumes, value):
    """sum over image pairs i < j of 2 |A_i n A_j| divided by the sum over the same pairs of |A_i| + |A_j|."""
    masks = [np.asarray(v) == value for v in volumes]
    num = den = 0
    for i in range(len(masks)):
        for j in range(i + 1, len(masks)):
            num += 2 * int((masks[i] & masks[j]).sum())
            den += int(masks[i].sum()) + int(masks[j].sum())
    return num / den
