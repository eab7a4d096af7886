"""frog_rank (include/frog_chain.h) restated in NumPy: (x, valid) per image from cover_restate.terms, the sort keys, np.sort
per voxel, then the quantile and MAD rules in float64 and float32, one operation per line, as the header states them."""
import numpy as np

import cover_restate

F4, F8, U4 = np.float32, np.float64, np.uint32
SENTINEL = U4(0xFFFFFFFF)
NAN_BITS = U4(0x7FC00000)


def keys_of(x):
    """The sort key of each float32: ~u where the sign bit of u = bits(x) is set, else u ^ 0x80000000."""
    u = np.ascontiguousarray(x, F4).view(U4)
    return np.where(u & U4(0x80000000) != 0, ~u, u ^ U4(0x80000000))


def values_of(keys):
    k = np.ascontiguousarray(keys, U4)
    return np.where(k & U4(0x80000000) != 0, k ^ U4(0x80000000), ~k).view(F4)


def entries(x, valid):
    """What an add keeps: the key where the voxel is valid and x is not NaN, 0xFFFFFFFF elsewhere."""
    return np.where(valid & ~np.isnan(x), keys_of(x), SENTINEL)


def value_at(a, k, q):
    """a: (P, V) float32, ascending along axis 0 over the first k[v] rows of column v; k >= 1 everywhere.  One float64
    operation per line; a NaN result is 0x7FC00000."""
    cols = np.arange(a.shape[1])
    with np.errstate(all="ignore"):
        h = F8(q) * (k - 1).astype(F8)
        fl = np.floor(h)
        f = h - fl
        lo = fl.astype(np.int64)
        hi = np.minimum(lo + 1, k - 1)
        alo, ahi = a[lo, cols], a[hi, cols]
        dlo, dhi = alo.astype(F8), ahi.astype(F8)
        diff = dhi - dlo
        part = f * diff
        total = dlo + part
        r = total.astype(F4)
    assert h.dtype == f.dtype == diff.dtype == part.dtype == total.dtype == F8 and r.dtype == F4
    r = np.where(np.isnan(r), NAN_BITS.view(F4), r)
    return np.where((f == 0) | (alo == ahi), alo, r)


def finish(planes, min_count=1, fill=0.0, quantiles=(0.5,)):
    """planes: (N,) + shape uint32 entries in add order.  Returns (values (n_q,) + shape float32, mad float32, count uint16)."""
    planes = np.asarray(planes, U4)
    shape = planes.shape[1:]
    keys = np.sort(planes.reshape(planes.shape[0], -1), axis=0)
    k = (keys != SENTINEL).sum(axis=0).astype(np.int64)
    enough = k >= min_count
    ks = np.maximum(k, 1)
    a = values_of(keys)
    out = np.empty((len(quantiles), keys.shape[1]), F4)
    for j, q in enumerate(quantiles):
        out[j] = np.where(enough, value_at(a, ks, q), F4(fill))
    m = value_at(a, ks, 0.5)
    with np.errstate(all="ignore"):
        d = np.abs(a - m[None, :])
    assert d.dtype == F4
    rows = np.arange(keys.shape[0])[:, None]
    dkeys = np.sort(np.where(rows < k[None, :], d.view(U4), SENTINEL), axis=0)
    mad = value_at(dkeys.view(F4), ks, 0.5)
    mad = np.where(np.isfinite(m), mad, NAN_BITS.view(F4))
    mad = np.where(enough, mad, F4(0))
    return out.reshape((len(quantiles),) + shape), mad.astype(F4).reshape(shape), k.astype(np.uint16).reshape(shape)


def collect(images, grid, interpolation=1, background=0.0, reslicer=cover_restate.reslice):
    """`images` as cover_restate.restate takes them: the (N,) + shape entries."""
    return np.stack([entries(*cover_restate.terms(links, volume, origin, spacing, grid, mask, interpolation, background, reslicer)[:2])
                     for links, volume, origin, spacing, mask in images])


def restate(images, grid, min_count=1, fill=0.0, quantiles=(0.5,), interpolation=1, background=0.0, reslicer=cover_restate.reslice):
    return finish(collect(images, grid, interpolation, background, reslicer), min_count, fill, quantiles)
