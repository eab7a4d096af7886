"""Connected components of a 3-D mask (frog_components, include/frog_chain.h) restated in NumPy: every set voxel starts with
its linear index as its label, each step takes the minimum over the neighbourhood's offsets among set voxels, and steps repeat
until nothing changes; a voxel then holds its component's smallest index, its root.  Ranking the roots gives the labels 1..K in
ascending order of root, the numbering of scipy.ndimage.label."""
import itertools

import numpy as np

NONE = np.int64(2 ** 62)


def offsets(connectivity):
    """The neighbours (dz, dy, dx) at connectivity 6, 18 or 26: those with at most 1, 2 or 3 coordinates that differ."""
    order = {6: 1, 18: 2, 26: 3}[connectivity]
    return [d for d in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(v != 0 for v in d) <= order]


def roots(mask, connectivity=26):
    """int64 on the grid: the smallest linear index of the voxel's component at a set voxel, NONE elsewhere."""
    on = np.asarray(mask) != 0
    nz, ny, nx = on.shape
    label = np.where(on, np.arange(on.size, dtype=np.int64).reshape(on.shape), NONE)
    offs = offsets(connectivity)
    while True:
        padded = np.full((nz + 2, ny + 2, nx + 2), NONE)
        padded[1:-1, 1:-1, 1:-1] = label
        best = label
        for dz, dy, dx in offs:
            best = np.minimum(best, padded[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx])
        best = np.where(on, best, NONE)
        if (best == label).all():
            return label
        label = best


def components(mask, connectivity=26):
    """(labels uint32, n, largest): labels 1..n in ascending order of root, 0 on unset voxels; the largest extent (0: empty)."""
    r = roots(mask, connectivity)
    on = r != NONE
    found, inverse, counts = np.unique(r[on], return_inverse=True, return_counts=True)
    labels = np.zeros(r.shape, np.uint32)
    labels[on] = inverse.reshape(-1) + 1
    return labels, len(found), int(counts.max()) if len(found) else 0
