"""frog_cover (include/frog_chain.h) restated in NumPy, composed from what is already pinned:
    value   = volume_restate.reslice(...) cast to float32 (the voxel frog_chain_reslice stores)
    inside  = the same function on an all-ones uint8 volume of the source's geometry, nearest, background 0
    mask    = the same function on (mask != 0) as uint8 on the mask's own geometry, nearest, background 0
then Welford's update and the finish in np.float32, one operation per line, as the device does them under
-ffp-contract=off.  Without a chain every voxel is inside and the value is the source's own voxel."""
import numpy as np

from volume_restate import reslice

F4 = np.float32


def terms(links, volume, origin, spacing, grid, mask=None, interpolation=1, background=0.0, reslicer=reslice):
    """(x float32, valid bool, resliced) of one image on `grid` = (dims(x, y, z), origin, spacing).  `links` None: no chain
    (the volume, and the mask array, are on the grid).  `mask`: None or (voxels, origin, spacing).  `reslicer(links, volume,
    origin, spacing, dims, grid_origin, grid_spacing, interpolation, background)` defaults to the NumPy restatement."""
    vol = np.ascontiguousarray(volume)
    if links is None:
        valid = np.ones(vol.shape, bool) if mask is None else (np.asarray(mask[0] if isinstance(mask, tuple) else mask) != 0)
        return vol.astype(F4), valid, vol
    r = reslicer(links, vol, origin, spacing, *grid, interpolation, background)
    valid = reslicer(links, np.ones(vol.shape, np.uint8), origin, spacing, *grid, 0, 0.0) != 0
    if mask is not None:
        m, mo, ms = mask
        valid = valid & (reslicer(links, (np.asarray(m) != 0).astype(np.uint8), mo, ms, *grid, 0, 0.0) != 0)
    return r.astype(F4), valid, r


def start(shape):
    return np.zeros(shape, F4), np.zeros(shape, F4), np.zeros(shape, np.uint16)


def update(state, x, valid):
    """k = count + 1; d = x - mean; mean = mean + d / (float)k; m2 = m2 + d * (x - mean); count = k, where valid."""
    mean, m2, count = state
    with np.errstate(all="ignore"):
        k = count.astype(np.uint32) + np.uint32(1)
        d = x - mean
        q = d / k.astype(F4)
        mean_new = mean + q
        e = x - mean_new
        t = d * e
        m2_new = m2 + t
    assert d.dtype == q.dtype == mean_new.dtype == e.dtype == t.dtype == m2_new.dtype == F4
    return np.where(valid, mean_new, mean), np.where(valid, m2_new, m2), np.where(valid, k, count).astype(np.uint16)


def finish(state, min_count=1, fill=0.0):
    """(mean, stdev, count): where count >= min_count the mean as held and sqrt(m2 / (float)count), elsewhere fill and 0."""
    mean, m2, count = state
    enough = count >= min_count
    with np.errstate(all="ignore"):
        variance = m2 / np.where(enough, count, 1).astype(F4)
        stdev = np.sqrt(variance)
    assert variance.dtype == stdev.dtype == F4
    return np.where(enough, mean, F4(fill)), np.where(enough, stdev, F4(0)), count.copy()


def restate(images, grid, min_count=1, fill=0.0, interpolation=1, background=0.0, reslicer=reslice):
    """`images`: (links or None, volume, origin, spacing, mask or None) per image, added in order."""
    state = start(tuple(int(d) for d in grid[0][::-1]))
    for links, volume, origin, spacing, mask in images:
        x, valid, _ = terms(links, volume, origin, spacing, grid, mask, interpolation, background, reslicer)
        state = update(state, x, valid)
    return finish(state, min_count, fill)
