"""frog_cover_score (include/frog_chain.h) and frog_score_metrics_from (include/frog_host.h) restated in NumPy, composed as
cover_restate.py composes:
    x, valid     = cover_restate.terms(...)            the value and the voxels frog_cover_add counts
    mean, count  = the state cover_restate.update(...) leaves
then the reference y in np.float64 (three operations), the bins in np.float32 (one operation per step), the six sums in the
ORDER the header states (tiles of 2048 voxels, thread t of 256 takes 2048 T + 256 j + t for ascending j, the wave's shuffle
tree as slices added pairwise, the four waves in ascending order, the tiles serially) and the metrics in the header's
operation order, in Python floats with math.log and math.sqrt (the C library's, as the host library uses them)."""
import math

import numpy as np

import cover_restate

F4, F8 = np.float32, np.float64
TILE, THREADS, ITEMS, WAVE = 2048, 256, 8, 64
SUMS = ("sx", "sy", "sxx", "syy", "sxy", "sad")


def reference(state, x, valid, min_count=1, leave_one_out=True):
    """(xd, y, counted, nonfinite): x as f64, the reference y, the voxels that enter the sums, those that go to n_nonfinite."""
    mean, _, count = state
    k = count.astype(np.uint32)
    takes = valid & (k >= max(2 if leave_one_out else 1, int(min_count)))
    xd = x.astype(F8)
    y = mean.astype(F8)
    if leave_one_out:
        with np.errstate(all="ignore"):
            mk = y * k.astype(F8)
            others = mk - xd
            y = others / np.where(takes, k - np.uint32(1), np.uint32(1)).astype(F8)
    assert y.dtype == F8
    finite = np.isfinite(xd) & np.isfinite(y)
    return xd, y, takes & finite, takes & ~finite


def bin_of(t, bins, lo, hi):
    """scale = (float)bins / (hi - lo); min(bins - 1, max(0, floorf((t - lo) * scale))), all float32, clamped as floats."""
    lo, hi = F4(lo), F4(hi)
    with np.errstate(all="ignore"):
        scale = F4(bins) / (hi - lo)
        d = np.asarray(t, F4) - lo
        f = np.floor(d * scale)
    assert scale.dtype == d.dtype == f.dtype == F4
    return np.where(~(f >= 0), F4(0), np.minimum(f, F4(bins - 1))).astype(np.int64)


def ordered_sum(terms):
    """The sum of a flat f64 array (0.0 where a voxel adds nothing: the sums never hold -0.0, so adding +0.0 is skipping) in
    the header's order."""
    terms = np.asarray(terms, F8).ravel()
    tiles = (len(terms) + TILE - 1) // TILE
    a = np.zeros(tiles * TILE, F8)
    a[:len(terms)] = terms
    a = a.reshape(tiles, ITEMS, THREADS // WAVE, WAVE)                  # voxel = 2048 T + 256 j + 64 w + l
    lanes = np.zeros((tiles, THREADS // WAVE, WAVE), F8)
    for j in range(ITEMS):                                              # 2. a thread's voxels in ascending j
        lanes = lanes + a[:, j]
    h = WAVE // 2
    while h:                                                            # 3. lanes l < h take lane l + h: 32, 16, 8, 4, 2, 1
        lanes = lanes[..., :h] + lanes[..., h:2 * h]
        h //= 2
    waves = lanes[..., 0]
    tile_sums = ((waves[:, 0] + waves[:, 1]) + waves[:, 2]) + waves[:, 3]   # 4.
    total = F8(0.0)
    for t in tile_sums:                                                 # 5.
        total = total + t
    return float(total)


def six_terms(xd, y, counted):
    """The per-voxel terms, one f64 operation each, 0.0 where the voxel is not counted."""
    with np.errstate(all="ignore"):
        diff = xd - y
        t = dict(sx=xd, sy=y, sxx=xd * xd, syy=y * y, sxy=xd * y, sad=np.abs(diff))
    return {name: np.where(counted, v, 0.0) for name, v in t.items()}


def score(state, x, valid, min_count=1, leave_one_out=True, bins=64, lo=0.0, hi=1.0):
    """The sums and the histogram frog_cover_score returns: a dict with n, n_nonfinite, the six sums and `histogram`
    ((bins, bins) uint64, or None for bins == 0)."""
    xd, y, counted, nonfinite = reference(state, x, valid, min_count, leave_one_out)
    out = dict(n=int(counted.sum()), n_nonfinite=int(nonfinite.sum()))
    for name, v in six_terms(xd, y, counted).items():
        out[name] = ordered_sum(v)
    out["histogram"] = None
    if bins:
        with np.errstate(all="ignore"):
            yf = y.astype(F4)
        cell = bin_of(x, bins, lo, hi) * bins + bin_of(yf, bins, lo, hi)
        out["histogram"] = np.bincount(cell[counted], minlength=bins * bins).astype(np.uint64).reshape(bins, bins)
    return out


def entropy(counts, n):
    acc = 0.0
    for c in counts:
        if c:
            p = float(c) / n
            t = p * math.log(p)
            acc = acc + t
    return -acc


def metrics(sums, histogram=None):
    """frog_score_metrics_from in the header's operation order, in Python floats."""
    nan = float("nan")
    out = dict(ncc=nan, mean_abs_diff=nan, rmse=nan, mi=nan, nmi=nan)
    if not sums["n"]:
        return out
    n = float(sums["n"])
    sx, sy, sxx, syy, sxy, sad = (float(sums[k]) for k in SUMS)
    cx = sxx - (sx * sx) / n
    cy = syy - (sy * sy) / n
    cxy = sxy - (sx * sy) / n
    if cx > 0 and cy > 0:
        out["ncc"] = cxy / math.sqrt(cx * cy)
    out["mean_abs_diff"] = sad / n
    r = ((sxx - 2 * sxy) + syy) / n
    out["rmse"] = 0.0 if r < 0 else math.sqrt(r)
    if histogram is None:
        return out
    h = np.asarray(histogram, np.uint64)
    rx, ry = h.sum(1, dtype=np.uint64), h.sum(0, dtype=np.uint64)
    hx, hy, hxy = entropy(rx.tolist(), n), entropy(ry.tolist(), n), entropy(h.ravel().tolist(), n)
    both = hx + hy
    out["mi"] = both - hxy
    out["nmi"] = 1.0 if hxy == 0 else both / hxy
    return out


def value_range(state, min_count=1):
    """The default histogram range: the smallest finite mean over the voxels with count >= min_count, the float32 after the
    largest."""
    mean, _, count = cover_restate.finish(state, min_count)
    v = mean[(count >= min_count) & np.isfinite(mean)]
    return float(v.min()), float(np.nextafter(v.max(), F4(np.inf)))


def robust_z(values):
    v = np.asarray(values, F8)
    s = np.sort(v[np.isfinite(v)])
    median = lambda a: a[len(a) // 2] if len(a) % 2 else (a[len(a) // 2 - 1] + a[len(a) // 2]) / 2.0
    mid = median(s)
    mad = median(np.sort(np.abs(s - mid)))
    return np.where(np.isfinite(v), (v - mid) / (1.4826 * mad) if mad > 0 else 0.0, np.nan)


def group_quality(images, grid, interpolation=1, min_count=1, bins=64, reslicer=cover_restate.reslice):
    """frog_amd.volume.group_quality restated: `images` as cover_restate.restate takes them; one dict per image."""
    state = cover_restate.start(tuple(int(d) for d in grid[0][::-1]))
    parts = []
    for links, volume, origin, spacing, mask in images:
        x, valid, _ = cover_restate.terms(links, volume, origin, spacing, grid, mask, interpolation, float(np.min(volume)), reslicer)
        state = cover_restate.update(state, x, valid)
        parts.append((x, valid))
    lo, hi = value_range(state, min_count)
    rows = []
    for x, valid in parts:
        s = score(state, x, valid, min_count, True, bins, lo, hi)
        s.update(metrics(s, s["histogram"]))
        rows.append(s)
    for row, z in zip(rows, robust_z([r["ncc"] for r in rows])):
        row["ncc_robust_z"] = float(z)
    return rows


# ---- the ranking case: six smooth volumes that coincide after known chains, one of them displaced --------------------------
RANK_GRID = ((19, 17, 13), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
RANK_SHAPE = (20, 24, 26)                                   # sources of 26 x 24 x 20 voxels, spacing 1, origin 0
RANK_OFFSETS = ((-3.5, -3.25, -3.0), (-2.75, -4.0, -3.5), (-4.25, -2.5, -2.75), (-3.0, -3.75, -4.0), (-3.75, -3.0, -3.25), (-2.5, -3.5, -3.75))
RANK_DISPLACED, RANK_SHIFT = 3, (3.0, -2.5, 2.0)            # image 3's chain lands several voxels off


def rank_scene(p0, p1, p2):
    """A smooth image in grid space: two blobs on a ramp, values around 0..1200."""
    blob = lambda c, w: np.exp(-((p0 - c[0]) ** 2 + (p1 - c[1]) ** 2 + (p2 - c[2]) ** 2) / (2.0 * w * w))
    return 200.0 + 20.0 * p0 + 10.0 * p1 + 900.0 * blob((6.0, 8.0, 5.0), 3.0) + 600.0 * blob((13.0, 6.0, 8.0), 2.5)


def ranking_group():
    """(images, grid): image k's voxel at source position q holds scene(q + offset_k), and its chain is p -> p - offset_k, so
    every image shows scene(p) at grid position p (plus a little noise of its own); image RANK_DISPLACED's chain is off by
    RANK_SHIFT."""
    from frog_amd.chain import Link
    rng = np.random.default_rng(71)
    z, y, x = np.meshgrid(*[np.arange(n, dtype=F8) for n in RANK_SHAPE], indexing="ij")
    images = []
    for k, off in enumerate(RANK_OFFSETS):
        vol = (rank_scene(x + off[0], y + off[1], z + off[2]) + rng.normal(0.0, 4.0, RANK_SHAPE)).astype(np.int16)
        M = np.eye(4)
        M[:3, 3] = [-v for v in off]
        if k == RANK_DISPLACED:
            M[:3, 3] += RANK_SHIFT
        images.append(([Link.linear(M)], vol, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), None))
    return images, RANK_GRID
