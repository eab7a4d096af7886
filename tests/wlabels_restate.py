"""frog_wlabels (include/frog_chain.h) restated in NumPy from the header's text: locally weighted label fusion of atlases
that are already on the target's grid.  Every line of the header is one NumPy operation in the stated precision, the patch
sums run over the (2 radius + 1)^3 offsets in z, y, x order, so the tests compare with ==."""
import numpy as np


def staged(volume, inside=None):
    """(x, valid): x = float32(volume) and valid = inside (default everywhere) and x finite -- t and validT, a and validA."""
    with np.errstate(over="ignore"):
        x = np.asarray(volume).astype(np.float32)
    valid = np.isfinite(x)
    if inside is not None:
        valid &= np.asarray(inside, bool)
    return x, valid


def weights(t, valid_t, a, valid_a, radius, power, floor):
    """(w float32, member bool) of one atlas.  Non-members are padded in around the grid and add +0.0 to every sum, which
    leaves the same bits as skipping them: every sum starts at +0.0 and no partial sum is -0.0."""
    r = int(radius)
    member = valid_t & valid_a
    m = np.pad(member, r).astype(np.float64)
    T = np.pad(np.where(member, t, np.float32(0)).astype(np.float64), r)
    A = np.pad(np.where(member, a, np.float32(0)).astype(np.float64), r)
    TT, AA, TA = T * T, A * A, T * A
    nz, ny, nx = t.shape
    n, st, sa, stt, saa, sta = (np.zeros(t.shape, np.float64) for _ in range(6))
    for dz in range(2 * r + 1):
        for dy in range(2 * r + 1):
            for dx in range(2 * r + 1):
                w = (slice(dz, dz + nz), slice(dy, dy + ny), slice(dx, dx + nx))
                n = n + m[w]; st = st + T[w]; sa = sa + A[w]; stt = stt + TT[w]; saa = saa + AA[w]; sta = sta + TA[w]
    cov = n * sta - st * sa
    vt = n * stt - st * st
    va = n * saa - sa * sa
    ok = (n >= 2) & (vt > 0) & (va > 0) & (cov > 0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q = ((cov * cov) / (vt * va)).astype(np.float32)
        c = np.sqrt(q)                                              # float32 in, float32 out: correctly rounded
    c = np.where(np.isfinite(c), np.minimum(c, np.float32(1)), c)
    c = np.where(ok, c, np.float32(0)).astype(np.float32)
    c = np.maximum(c, np.float32(floor))
    w = c
    for _ in range(int(power) - 1):
        w = w * c
    assert w.dtype == np.float32
    return w, member


def restate(target, atlases, radius, power, floor, fill_label=0, target_inside=None):
    """target: array on the grid; atlases: (image, labels) or (image, labels, inside) per atlas in call order, all on the
    grid (`inside`: where the reslice's inside test held; default everywhere).  Returns values (int64 ascending: every value
    an atlas' label map holds), scores[l] (float32), total, labels (int64; fill_label where total == 0), confidence."""
    t, valid_t = staged(target, target_inside)
    label_maps = [np.asarray(at[1]).astype(np.int64) for at in atlases]
    values = np.unique(np.concatenate([l.ravel() for l in label_maps]))
    scores = np.zeros((len(values),) + t.shape, np.float32)
    for at, lab in zip(atlases, label_maps):
        a, valid_a = staged(at[0], at[2] if len(at) > 2 else None)
        w, member = weights(t, valid_t, a, valid_a, radius, power, floor)
        idx = np.searchsorted(values, lab)
        for l in range(len(values)):
            hit = member & (idx == l)
            scores[l] = np.where(hit, scores[l] + w, scores[l])
    total = np.zeros(t.shape, np.float32)
    best = np.zeros(t.shape, np.float32)
    winner = np.zeros(t.shape, np.int64)
    for l in range(len(values)):
        total = total + scores[l]
        better = scores[l] > best                                   # strictly larger than every earlier one, and > 0
        best = np.where(better, scores[l], best)
        winner = np.where(better, l, winner)
    some = total != 0
    with np.errstate(divide="ignore", invalid="ignore"):
        confidence = np.where(some, best / total, np.float32(0)).astype(np.float32)
    return {"values": values, "scores": scores, "total": total, "labels": np.where(some, values[winner], np.int64(fill_label)),
            "confidence": confidence}


def probability(r, value):
    """score / total per voxel in float32, 0 where total == 0."""
    l = int(np.searchsorted(r["values"], value))
    assert r["values"][l] == value
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(r["total"] != 0, r["scores"][l] / r["total"], np.float32(0)).astype(np.float32)
