"""frog_cover_score's restatement (score_restate.py) and frog_score_metrics_from (include/frog_host.h) without a device: the
stated summation order against math.fsum, the host metrics against the restatement, entropy identities, every NaN and zero
rule, the float32 bin edges, the ranking case the GPU test reuses, and bin/AverageImage's -q flag errors."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from frog_amd import _abi

import cover_restate
import score_restate
from test_cover import _random_group

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")
U = 2.0 ** -53                      # unit roundoff of float64
METRIC_BOUND = 64 * 2.0 ** -52      # times max(1, |value|): a handful of operations per metric, <= 4096 entropy terms


def host_metrics(sums, histogram=None):
    """frog_score_metrics_from on a dict of sums and a (bins, bins) uint64 array."""
    s = _abi.FrogScoreSums()
    for name, _ in s._fields_:
        setattr(s, name, sums.get(name, 0))
    m = _abi.FrogScoreMetrics()
    h = None if histogram is None else np.ascontiguousarray(histogram, np.uint64)
    rc = _abi.host_lib().frog_score_metrics_from(C.byref(s), None if h is None else h.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                 0 if h is None else h.shape[0], C.byref(m))
    assert rc == _abi.FROG_OK
    return {name: getattr(m, name) for name, _ in m._fields_}


def close(got, want, bound=METRIC_BOUND):
    if math.isnan(want):
        return math.isnan(got)
    return abs(got - want) <= bound * max(1.0, abs(want))


def test_ordered_sums_stay_within_the_naive_bound_of_fsum():
    """Any order of n additions stays within n * 2^-53 * sum |term| of the exact sum (Higham, Accuracy and Stability, 4.2: the
    recursive bound (n - 1) u / (1 - (n - 1) u); a tree's depth is smaller).  Sizes: less than one wave, one tile exactly, a
    partial last tile and a partial last wave (the GPU test's 4199), several tiles."""
    rng = np.random.default_rng(3)
    for n in (1, 37, 2048, 4199, 3 * 2048 + 1):
        for terms in (rng.normal(0, 1e3, n), rng.uniform(0, 1, n) * 10.0 ** rng.integers(-8, 8, n), np.abs(rng.normal(0, 1, n))):
            got = score_restate.ordered_sum(terms)
            exact = math.fsum(terms.tolist())
            assert abs(got - exact) <= n * U * math.fsum(np.abs(terms).tolist()), n
    assert score_restate.ordered_sum(np.zeros(5)) == 0.0 and math.copysign(1.0, score_restate.ordered_sum(np.zeros(5))) == 1.0
    # the order is the stated one, not another: lane 0 + lane 32 first
    t = np.zeros(2048)
    t[0], t[32], t[1] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert score_restate.ordered_sum(t) == 1.0                      # (1 + 2^-53) rounds to 1 before lane 1's term arrives
    t[32], t[33] = 0.0, 2.0 ** -53
    assert score_restate.ordered_sum(t) == 1.0 + 2.0 ** -52         # lanes 1 and 33 meet first: 2^-52 survives


def test_restated_score_of_a_group():
    """The restatement on the groups of test_cover.py: the sums against f64 sums of the same terms, n against the counts."""
    for seed, n_images, dtype in ((1, 6, "int16"), (2, 5, "float32")):
        images, grid = _random_group(seed, n_images, dtype)
        state = cover_restate.start(grid[0][::-1])
        parts = []
        for l, v, o, s, m in images:
            x, valid, _ = cover_restate.terms(l, v, o, s, grid, m)
            state = cover_restate.update(state, x, valid)
            parts.append((x, valid))
        lo, hi = score_restate.value_range(state)
        for loo in (True, False):
            for min_count in (1, 2, 3):
                x, valid = parts[2]
                got = score_restate.score(state, x, valid, min_count, loo, 16, lo, hi)
                need = max(2 if loo else 1, min_count)
                takes = valid & (state[2] >= need)
                assert got["n"] == int(takes.sum()) > 0 and got["n_nonfinite"] == 0
                assert int(got["histogram"].sum()) == got["n"]
                xd, y, counted, _ = score_restate.reference(state, x, valid, min_count, loo)
                for name, terms in score_restate.six_terms(xd, y, counted).items():
                    exact = math.fsum(terms.ravel().tolist())
                    assert abs(got[name] - exact) <= terms.size * U * math.fsum(np.abs(terms).ravel().tolist()), name
                if not loo:
                    assert np.array_equal(y[counted], state[0].astype(np.float64)[counted])
        # leave-one-out is the mean of the others up to the f32 rounding of Welford's mean: |m - exact| <= (n + 4 H_n) u M
        # (test_cover.py), times k / (k - 1) <= 2, plus three f64 roundings
        xs = np.stack([p[0] for p in parts]).astype(np.float64)
        vs = np.stack([p[1] for p in parts])
        x, valid = parts[0]
        xd, y, counted, _ = score_restate.reference(state, x, valid, 1, True)
        others = (np.where(vs, xs, 0).sum(0) - xd) / np.maximum(vs.sum(0) - 1, 1)
        M = float(np.abs(xs).max())
        bound = 2 * (n_images + 4 * (1 + math.log(n_images))) * 2.0 ** -24 * M * 1.01
        assert counted.any() and (np.abs(y - others)[counted] <= bound).all()


def random_sums(rng, n=5000):
    x = rng.normal(300, 80, n)
    y = 0.7 * x + rng.normal(0, 30, n)
    return dict(n=n, n_nonfinite=0, sx=x.sum(), sy=y.sum(), sxx=(x * x).sum(), syy=(y * y).sum(), sxy=(x * y).sum(),
                sad=np.abs(x - y).sum()), x, y


def test_host_metrics_equal_the_restatement():
    rng = np.random.default_rng(5)
    for bins in (2, 7, 64):
        sums, x, y = random_sums(rng)
        lo, hi = float(min(x.min(), y.min())), float(max(x.max(), y.max())) + 1.0
        cell = score_restate.bin_of(x, bins, lo, hi) * bins + score_restate.bin_of(y, bins, lo, hi)
        h = np.bincount(cell, minlength=bins * bins).astype(np.uint64).reshape(bins, bins)
        got, want = host_metrics(sums, h), score_restate.metrics(sums, h)
        for name in want:
            assert close(got[name], want[name]), (bins, name, got[name], want[name])
        # and they are what they claim to be, against NumPy's own (looser: another formula)
        assert abs(got["ncc"] - np.corrcoef(x, y)[0, 1]) < 1e-9
        assert abs(got["rmse"] - math.sqrt(np.mean((x - y) ** 2))) < 1e-9 * got["rmse"]
        assert abs(got["mean_abs_diff"] - np.mean(np.abs(x - y))) < 1e-12 * got["mean_abs_diff"]
        assert 0 < got["mi"] and 1 < got["nmi"] < 2


def test_entropy_identities():
    """Bound, u = 2^-53: an entropy of T non-empty bins sums T terms p log p, each with at most 3 roundings (quotient, log,
    product), into partial sums <= H <= log T, so its error is at most (T + 3) u H.  The check allows 64 * 2^-52 = 128 u times
    max(1, |value|).
    Bijective re-binning, 16 bins (H <= log 16 = 2.78): three entropies of 16 terms and two more operations on values <= 5.6,
    3 * 19 u * 2.78 + 2 u * 5.6 = 170 u, within 128 u * H(x) for H(x) > 1.33, which the test asserts.  (With 64 bins the
    worst case, 840 u against 532 u, would not be covered by the derivation.)
    Product histogram, 4 x 4 (the value is 0, so 128 u in all): H(h) of 16 terms <= 19 u * 2.78 = 53 u, H(rx) and H(ry) of
    4 terms <= 7 u * 1.39 = 10 u each, the sum and the difference 2 u * 2.78: 79 u."""
    rng = np.random.default_rng(7)
    bins = 16
    counts = rng.integers(1, 1000, bins).astype(np.uint64)
    perm = rng.permutation(bins)
    h = np.zeros((bins, bins), np.uint64)
    h[np.arange(bins), perm] = counts                               # y's bin is a bijection of x's
    n = int(counts.sum())
    got = host_metrics(dict(n=n), h)
    hx = score_restate.entropy(counts.tolist(), float(n))
    assert close(got["mi"], hx) and close(got["nmi"], 2.0) and hx > 1.33
    # the same inside a 64-bin histogram: the empty bins are skipped
    big = np.zeros((64, 64), np.uint64)
    big[::4, ::4] = h
    got = host_metrics(dict(n=n), big)
    assert close(got["mi"], hx) and close(got["nmi"], 2.0)
    # product histogram: independent, mi == 0 and nmi == 1
    a, b = rng.integers(1, 50, 4).astype(np.uint64), rng.integers(1, 50, 4).astype(np.uint64)
    prod = np.outer(a, b).astype(np.uint64)
    got = host_metrics(dict(n=int(prod.sum())), prod)
    assert close(got["mi"], 0.0) and close(got["nmi"], 1.0)
    sparse = np.zeros((64, 64), np.uint64)
    sparse[3:63:15, 1:61:15] = prod
    got = host_metrics(dict(n=int(prod.sum())), sparse)
    assert close(got["mi"], 0.0) and close(got["nmi"], 1.0)


def test_nan_and_zero_rules():
    nan = math.isnan
    h = np.zeros((4, 4), np.uint64)
    m = host_metrics(dict(n=0), h)                                  # n == 0: everything NaN
    assert all(nan(v) for v in m.values())
    assert all(nan(v) for v in score_restate.metrics(dict(n=0, sx=0, sy=0, sxx=0, syy=0, sxy=0, sad=0), h).values())
    sums, x, y = random_sums(np.random.default_rng(9), 100)
    m = host_metrics(sums, None)                                    # no histogram: mi and nmi NaN, the rest as usual
    assert nan(m["mi"]) and nan(m["nmi"]) and not nan(m["ncc"]) and m["rmse"] > 0 and m["mean_abs_diff"] > 0
    want = score_restate.metrics(sums, None)
    assert nan(want["mi"]) and nan(want["nmi"]) and close(m["ncc"], want["ncc"])
    # a constant x: the variance is 0 (or rounds negative), ncc NaN; everything in one bin: H(x, y) == 0 and nmi == 1
    const = dict(n=10, sx=30.0, sy=float(np.arange(10).sum()), sxx=90.0, syy=float((np.arange(10) ** 2).sum()),
                 sxy=float(3 * np.arange(10).sum()), sad=float(np.abs(3 - np.arange(10)).sum()))
    h[1, 2] = 10
    m = host_metrics(const, h)
    assert nan(m["ncc"]) and m["nmi"] == 1.0 and m["mi"] == 0.0 and m["mean_abs_diff"] == const["sad"] / 10
    negative = dict(const, sxx=89.0)                                # sxx - sx^2 / n < 0
    assert nan(host_metrics(negative, h)["ncc"]) and nan(score_restate.metrics(negative, h)["ncc"])
    # x == y: the radicand sxx - 2 sxy + syy is 0; rounded below it the rmse is 0, not NaN
    same = dict(n=3, sx=6.0, sy=6.0, sxx=14.0, syy=14.0, sxy=14.0, sad=0.0)
    assert host_metrics(same)["rmse"] == 0.0 and host_metrics(same)["ncc"] == 1.0
    below = dict(same, sxy=14.0 + 2.0 ** -48)
    assert host_metrics(below)["rmse"] == 0.0 and score_restate.metrics(below)["rmse"] == 0.0
    # bad arguments
    lib = _abi.host_lib()
    s, out = _abi.FrogScoreSums(), _abi.FrogScoreMetrics()
    hp = h.ctypes.data_as(C.POINTER(C.c_uint64))
    assert lib.frog_score_metrics_from(None, hp, 4, C.byref(out)) == _abi.FROG_E_INVALID
    assert lib.frog_score_metrics_from(C.byref(s), hp, 4, None) == _abi.FROG_E_INVALID
    assert lib.frog_score_metrics_from(C.byref(s), hp, 1, C.byref(out)) == _abi.FROG_E_INVALID
    assert lib.frog_score_metrics_from(C.byref(s), hp, 65, C.byref(out)) == _abi.FROG_E_INVALID


def test_bin_edges_in_float32():
    f4 = np.float32
    lo, hi, bins = -3.5, 12.25, 7
    below_hi = np.nextafter(f4(hi), f4(-np.inf))
    t = np.array([lo, below_hi, hi, np.nextafter(f4(hi), f4(np.inf)), 1e30, np.inf, np.nextafter(f4(lo), f4(-np.inf)), -1e30, -np.inf], f4)
    assert score_restate.bin_of(t, bins, lo, hi).tolist() == [0, bins - 1, bins - 1, bins - 1, bins - 1, bins - 1, 0, 0, 0]
    # u8 values, lo = 0, hi = 256, 64 bins: scale = 0.25 exactly, the bin is v // 4
    v = np.arange(256)
    assert score_restate.bin_of(v.astype(f4), 64, 0.0, 256.0).tolist() == (v // 4).tolist()
    # every float of a binade edge lands in a valid bin, monotonically
    grid = np.linspace(-5, 14, 4001).astype(f4)
    b = score_restate.bin_of(grid, bins, lo, hi)
    assert b.min() == 0 and b.max() == bins - 1 and (np.diff(b) >= 0).all() and set(b.tolist()) == set(range(bins))


def test_the_displaced_image_ranks_last_in_the_restatement():
    """The inputs of test_gpu_score.py's ranking test: the condition holds for the reference before it is asked of the device."""
    images, grid = score_restate.ranking_group()
    rows = score_restate.group_quality(images, grid)
    k = score_restate.RANK_DISPLACED
    assert all(r["n"] == int(np.prod(grid[0])) for r in rows)                      # every image covers the grid
    for name in ("ncc", "nmi"):
        order = sorted(range(len(rows)), key=lambda i: rows[i][name])
        assert order[0] == k, (name, [r[name] for r in rows])
    others = [r["ncc"] for i, r in enumerate(rows) if i != k]
    assert rows[k]["ncc"] < min(others) - 0.05 and min(others) > 0.9 and rows[k]["ncc_robust_z"] < -3
    assert rows[k]["rmse"] == max(r["rmse"] for r in rows) and rows[k]["mean_abs_diff"] == max(r["mean_abs_diff"] for r in rows)


def test_quality_flag_errors(tmp_path):
    exe = os.path.join(BIN, "AverageImage")

    def run(*args):
        return subprocess.run([exe, "bbox.json", "2", "a.nii.gz", "b.nii.gz", "c.nii.gz", "-o", "out", *args], cwd=tmp_path,
                              capture_output=True, text=True, timeout=60)

    r = subprocess.run([exe, "bbox.json", "2"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "[-q 1 [-qb bins] [-qr lo hi]]" in r.stdout
    for args in (("-q", "1"), ("-q", "1", "-c", "0"), ("-q", "1", "-qb", "32")):
        r = run(*args)
        assert r.returncode == 1 and "needs -c 1" in r.stdout, (args, r.stdout)
    for args in (("-c", "1", "-qb", "32"), ("-c", "1", "-qr", "0", "100"), ("-c", "1", "-q", "0", "-qb", "8")):
        r = run(*args)
        assert r.returncode == 1 and "need -q 1" in r.stdout, (args, r.stdout)
    for args in (("-qb", "1"), ("-qb", "65"), ("-qr", "5", "5"), ("-qr", "7", "2"), ("-qr", "0", "inf"), ("-qr", "nan", "1")):
        r = run("-c", "1", "-q", "1", *args)
        assert r.returncode == 1 and args[0] in r.stdout, (args, r.stdout)
    assert not (tmp_path / "out").exists()
