"""The culling list's certificate (frog_amd/csrc/device/k_cull.hip.h) restated in numpy, line for line: the per-image cutoff
of both stages, the rule that lists a half-link, the displacement a list allows and the check that declares it stale.
The cutoffs are f64 searches stored as f32 (they explain a device value; the tests' criterion is what the cutoff certifies);
the list rule, the allowance and the check are f32 expressions, restated with every product and sum rounded to f32."""
import numpy as np

F = np.float32
INF = F(np.inf)


def mixture_probability(d, c1, c2, ratio):
    """mixture_probability: Stats::getInlierProbability in f64, real-valued form.  d may be an array."""
    eps, c = 1e-10, 0.797884560802865
    d = np.asarray(d, np.float64)
    a, b = d / (c1 + eps), d / (c2 + eps)
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        x1 = ratio * c * a * a * np.exp(-0.5 * a * a) / (c1 + eps)
        x2 = (1.0 - ratio) * c * b * b * np.exp(-0.5 * b * b) / (c2 + eps)
        return x1 / (x1 + x2 + eps)


def degenerate(em, threshold):
    """The mixtures (f32 c1, c2, ratio) and thresholds for which cull_cutoff_of gives no cutoff."""
    c1, c2, r = (float(F(v)) for v in em)
    return not (F(threshold) >= F(1e-3) and c1 > 0.0 and c2 > c1 and r > 0.0 and r < 1.0 and c2 < 1e30)


def cull_cutoff_of(em, threshold):
    """cull_cutoff_of: bracket by doubling from sqrt(2) c1, 32 bisections, the certified side, rounded up into f32."""
    if degenerate(em, threshold):
        return INF
    c1, c2, r = (float(F(v)) for v in em)
    target = 0.5 * float(F(threshold))
    lo = max(1.4142135623730951 * (c1 + 1e-10) * 1.000001, 0.2)
    out = INF
    if mixture_probability(lo, c1, c2, r) <= target:
        out = F(lo)
    else:
        hi, found = lo, False
        for _ in range(200):
            hi *= 2.0
            found = bool(mixture_probability(hi, c1, c2, r) <= target)
            if found:
                break
        if found:
            for _ in range(32):
                mid = 0.5 * (lo + hi)
                if mixture_probability(mid, c1, c2, r) <= target:
                    hi = mid
                else:
                    lo = mid
            out = F(hi)
    if out < INF:
        out = F(F(out * F(1.000001)) + F(1e-6))
    return out


def em_derived_of(em):
    """k_stats.hip.h em_derived_of: (kq1, kq2, s1, s2) in f32, product by product."""
    eps, c, K = F(1e-10), F(0.797884560802865), F(-0.72134752044448170368)
    c1, c2, r = F(em[0]), F(em[1]), F(em[2])
    with np.errstate(all="ignore"):
        inv1, inv2 = F(F(1.0) / F(c1 + eps)), F(F(1.0) / F(c2 + eps))
        q1, q2 = F(inv1 * inv1), F(inv2 * inv2)
        kq1 = F(F(F(r * c) * inv1) * q1)
        kq2 = F(F(F(F(F(1.0) - r) * c) * inv2) * q2)
        return kq1, kq2, F(q1 * K), F(q2 * K)


def cull_cutoff_linear_of(em):
    """cull_cutoff_linear_of: the distance from which the linear sweep's f32 weight is exactly +0."""
    kq1, kq2, s1, _ = em_derived_of(em)
    s = -float(s1)
    if not (s > 0.0) or not (s < 1e30):
        return INF
    if not (kq1 >= 0) or not (kq2 >= 0) or not (kq1 < INF) or not (kq2 < INF):
        return INF
    c = F(np.sqrt(160.0 / s))
    return max(F(F(c * F(1.00001)) + F(1e-6)), F(0.2))


def link_d2(xyz2, a, b):
    """The sweep's squared distance of the links (a[i], b[i]): dx*dx + dy*dy + dz*dz in f32, no contraction."""
    x = np.asarray(xyz2, F)
    with np.errstate(all="ignore"):
        d = x[np.asarray(b)] - x[np.asarray(a)]             # f32 - f32 -> f32
        dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
        return ((dx * dx).astype(F) + (dy * dy).astype(F)).astype(F) + (dz * dz).astype(F)


def listed(d2, cutA, cutB):
    """The list rule of cull_build_kernel and of the sweep's own list-writing form: ~(d2 >= min(cutA, cutB)^2) in f32 -- a
    NaN distance is listed, an infinite cutoff lists everything -- and an infinite distance is listed whatever the cutoff
    (the weight there is inf * 0 = NaN, on the device as in the reference: nothing is certified about it)."""
    d2 = np.asarray(d2, F)
    with np.errstate(all="ignore"):
        cut = np.minimum(np.asarray(cutA, F), np.asarray(cutB, F))
        return ~((d2 >= (cut * cut).astype(F)) & (d2 < INF))


def list_cutoff(cut_now, scale, pad):
    """cull_list_cutoff_kernel: scale * cut_now + pad in f32 (inf stays inf)."""
    with np.errstate(all="ignore"):
        return (F(scale) * np.asarray(cut_now, F)).astype(F) + F(pad)


def allowance(cut_now, cut_list):
    """cull_allow_kernel: min over the images that have a cutoff of (list 0.99999 - (now 1.0001 + 0.01)) / 2, -1 once a term is
    NaN, a shade below the bound (- |a| 1e-6)."""
    now, lst = np.asarray(cut_now, F), np.asarray(cut_list, F)
    assert now.size <= 256              # one image per thread: a NaN term is -1 on its thread, fminf folds the threads' values
    with np.errstate(all="ignore"):
        v = (F(0.5) * ((lst * F(0.99999)).astype(F) - ((now * F(1.0001)).astype(F) + F(0.01)).astype(F)).astype(F)).astype(F)
        v = np.where(v == v, v, F(-1.0)).astype(F)
        v = v[~((now == INF) & (lst == INF))]
        a = F(v.min()) if v.size else INF
        return F(a - F(abs(a) * F(1e-6)))


def disp_of(xyz2, snap):
    """cull_disp_kernel: the largest f32 distance of a point from the snapshot, by the bits (a NaN is above every number)."""
    u, v = np.asarray(xyz2, F), np.asarray(snap, F)
    with np.errstate(all="ignore"):
        d = u - v
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        s = ((dx * dx).astype(F) + (dy * dy).astype(F)).astype(F) + (dz * dz).astype(F)
        dist = np.sqrt(s).astype(F)
    bits = dist.view(np.uint32) & np.uint32(0x7FFFFFFF)
    return np.array([bits.max() if bits.size else 0], np.uint32).view(F)[0]


def stale(cut_now, cut_list, D):
    """cull_validate_kernel: True (state 1) unless now 1.0001 + 0.01 + 2 D <= list 0.99999 for every image, in f32; a NaN
    anywhere is stale."""
    now, lst, D = np.asarray(cut_now, F), np.asarray(cut_list, F), F(D)
    with np.errstate(all="ignore"):
        need = ((now * F(1.0001)).astype(F) + F(0.01)).astype(F) + F(F(2.0) * D)
        have = (lst * F(0.99999)).astype(F)
        return bool(np.any(~(need <= have)))
