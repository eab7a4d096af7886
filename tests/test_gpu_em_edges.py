"""em_scan_kernel (k_stats.hip.h), the prefix-sum form of Stats::estimateDistribution's accumulators, where its argument hands
a term to the real arithmetic: exact ties on odd and even sums, near ties of the f64 chains, binade exits at lane 0, at lane 63,
twice in a batch and on the power of two itself, S + T = 2^24 - 1 and 2^24, zero, denormal and non-finite sums, batches past
EM_GUESS_BATCHES, and guesses gone stale.  The cases and the census that shows each contains its event are
tests/em_restate.py's (checked on the CPU by tests/test_em_restate.py).

Forcing the samples: two-image groups, every point of the even image at the origin and point j of the odd image at
(d_j, 0, 0), one link per point: both images retain sample j = d_j.  All cases of a context are consecutive image pairs, so
one refresh fits them all in one launch.  The samples fed to the oracle are the ones read back, not the intended ones.

Five fits of every image from the same start parameters must have the same bits:
    first   updateStats()                 em_scan_kernel in a fresh context: the guesses it holds are empty
    warm    updateStats() again           em_scan_kernel with the guesses the first refresh left, batch by batch
    cold    frog_test_em_refit(ctx, 0)    em_scan_kernel without guesses
    term    frog_test_em_refit(ctx, 1)    em_kernel, term by term
    oracle  Stats("oracle"), and Stats("ref") where oracle/_ref is built
term == oracle and warm or cold different: the scan form is wrong.  term != oracle: the membership differs (device exp)."""
import numpy as np
import pytest

import em_restate as er
from frog_amd import _abi
from frog_amd.image_group import ImageGroup, device_inlier_probability
from frog_amd.pairs import Pairs
from oracle.oracle_api import OracleGroup, Stats, ref_lib
from em_restate import oracle_fit, same
from gpu_util import INLIER_PROBABILITY_BOUND as BOUND

pytestmark = pytest.mark.gpu
CASES = er.all_cases()
CONTEXTS = {cap: [c for c in CASES if c["cap"] == cap] for cap in sorted({c["cap"] for c in CASES})}    # one per iteration cap


def group_of(coords, **opt):
    """Image 2k: len(coords[k]) points at the origin; image 2k + 1: point j at (coords[k][j], 0, 0); link j -- j."""
    sizes = [len(c) for c in coords for _ in (0, 1)]
    po = np.concatenate([[0], np.cumsum(sizes)])
    pairs = Pairs.from_arrays(po, positions(coords), [(2 * k, 2 * k + 1, np.arange(len(c)), np.arange(len(c)))
                                                      for k, c in enumerate(coords)])
    g = ImageGroup(pairs, **opt)
    g.setupLinearTransforms()
    g.transformPoints()
    return pairs, g


def positions(coords):
    out = []
    for c in coords:
        odd = np.zeros((len(c), 3), np.float32)
        odd[:, 0] = c
        out += [np.zeros((len(c), 3), np.float32), odd]
    return np.concatenate(out)


def refresh(g, starts, cap, refits=True):
    """One statistics refresh from `starts` (one per image): {"warm", "cold", "term", "oracle", "ref", "samples"} per image."""
    n = len(starts)
    lib = _abi.hip_lib()

    def restart():
        for i in range(n):
            g.set_em(i, starts[i])
    restart()
    g.updateStats()
    out = {"warm": [g.em(i).copy() for i in range(n)], "samples": [g.samples(i)[0] for i in range(n)]}
    if refits:
        for name, term_by_term in (("cold", 0), ("term", 1)):
            restart()
            assert lib.frog_test_em_refit(g._ctx, term_by_term) == _abi.FROG_OK
            out[name] = [g.em(i).copy() for i in range(n)]
        for i in range(n):                                  # leave the context as the refresh left it
            g.set_em(i, out["warm"][i])
    out["oracle"] = [oracle_fit("oracle", out["samples"][i], starts[i], cap) for i in range(n)]
    out["ref"] = [oracle_fit("ref", out["samples"][i], starts[i], cap) for i in range(n)] if ref_lib() is not None else None
    return out


def verdict(r, i, what):
    """The comparison of one image, with the message the forms' roles give it."""
    warm, oracle = r["warm"][i], r["oracle"][i]
    msg = f"{what}: warm {warm} oracle {oracle}"
    if "first" in r:
        assert same(r["first"][i], oracle), f"the SCAN FORM is wrong (first refresh of the context) -- {what}: {r['first'][i]} oracle {oracle}"
    if "term" in r:
        cold, term = r["cold"][i], r["term"][i]
        msg = f"{what}: warm {warm} cold {cold} term-by-term {term} oracle {oracle}"
        assert same(term, oracle), "the MEMBERSHIP differs (em_kernel against the oracle: device exp against libm) -- " + msg
        assert same(cold, term), "the SCAN FORM is wrong (cold guesses; em_kernel and the oracle agree) -- " + msg
    assert same(warm, oracle), "the SCAN FORM is wrong (warm guesses: the product path) -- " + msg
    if r["ref"] is not None:
        assert same(oracle, r["ref"][i]), f"{what}: the oracle {oracle} and the reference build {r['ref'][i]} differ"


@pytest.fixture(scope="module")
def fits():
    """Every case of every context fitted once: {case name: (refresh result, image of the even side, iteration cap)}."""
    out, keep = {}, {}
    for cap, cases in CONTEXTS.items():
        size = max(len(c["samples"]) for c in cases)        # equals the largest count, exceeds every other
        pairs, g = group_of([c["coordinates"] for c in cases], stats_max_size=size, stats_max_iterations=cap)
        g.set_points2(positions([c["coordinates"] for c in cases]))
        starts = [c["start"] for c in cases for _ in (0, 1)]
        first = refresh(g, starts, cap, refits=False)["warm"]
        r = refresh(g, starts, cap)                          # the same samples and starts, now on persisted guesses
        r["first"] = first
        for k, c in enumerate(cases):
            out[c["name"]] = (r, 2 * k, cap)
        keep[cap] = (pairs, g, cases, r)
    out["_contexts"] = keep
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_four_fits_have_the_same_bits(case, fits):
    r, image, _ = fits[case["name"]]
    for i in (image, image + 1):
        # what the census of tests/test_em_restate.py was taken on is what the device retained
        assert np.array_equal(r["samples"][i], case["samples"]), f"{case['name']}: image {i} retained other samples than intended"
        verdict(r, i, f"{case['name']} image {i} ({len(case['samples'])} samples, start {case['start']})")


def test_stale_guesses():
    """The product path only: four refreshes in one context with the odd images' coordinates multiplied by 2^7, 2^-12 and 3
    in between (every guess of every batch is then wrong by 7, 5 and one or two binades), every third image restarted far
    from its fit, one image pair going from all-zero samples to ordinary ones and back: after every refresh updateStats()
    equals the oracle from the same start on the samples read back."""
    counts = (129, 8193, 700, 16385, 8192, 2000, 65, 66000, 4000)
    base = [er.two_scale(n, 500 + n) for n in counts]
    flip = len(counts) - 1                                   # this pair: zeros, ordinary, zeros, ordinary
    pairs, g = group_of(base, stats_max_size=max(counts))
    far = [(1e-3, 1e4, 0.01), (500.0, 0.5, 0.99), er.T0, (1e-6, 1e-6, 1e-6)]
    scale = np.float32(1.0)
    for k, factor in enumerate((1.0, 2.0 ** 7, 2.0 ** -12, 3.0)):
        scale = np.float32(scale * np.float32(factor))
        coords = [b * scale for b in base]
        if k % 2 == 0:
            coords[flip] = np.zeros_like(base[flip])
        g.set_points2(positions(coords))
        starts = [far[k] if i % 3 == 0 else g.em(i).copy() for i in range(2 * len(counts))]
        r = refresh(g, starts, 10000, refits=False)
        for i in range(2 * len(counts)):
            assert np.array_equal(r["samples"][i], coords[i // 2]), f"refresh {k} image {i}: retained other samples than intended"
            verdict(r, i, f"refresh {k} (coordinates x {float(scale)}), image {i} ({counts[i // 2]} samples, start {starts[i]})")


def finite_mixtures(fits):
    seen = {}
    for name, v in fits.items():
        if name == "_contexts":
            continue
        r, image, _ = v
        for i in (image, image + 1):
            e = r["warm"][i]
            if np.all(np.isfinite(e)):
                seen[e.tobytes()] = (name, e)
    return list(seen.values())


def test_inlier_probability_of_the_fitted_mixtures(fits):
    """Downstream of the fits: every finite mixture the cases end in -- the clamped ones among them, c1 = epsilon,
    ratio = epsilon, c2 of 1e5 -- through the sweep's inlier weight at about 200 distances: the form with the reference's
    promotions has Stats.prob's bits, the fast form stays inside the derived bound."""
    mixtures = finite_mixtures(fits)
    assert any(e[0] == np.float32(1e-6) for _, e in mixtures) and any(e[2] == np.float32(1e-6) for _, e in mixtures)
    assert any(e[1] > 1e5 for _, e in mixtures) and len(mixtures) >= 20
    worst = (0.0, None)
    for name, e in mixtures:
        d = np.concatenate([e[0] * np.geomspace(0.02, 60.0, 90), e[1] * np.geomspace(0.02, 60.0, 90),
                            np.linspace(0.0, 0.2, 21)]).astype(np.float32)
        d2 = (d * d).astype(np.float32)
        d2 = d2[np.isfinite(d2)]
        s = Stats("oracle")
        s.set_params(e)
        want = np.array([s.prob(x) for x in np.sqrt(d2)], np.float32)
        fast, exact = device_inlier_probability(e, d2)
        assert np.array_equal(exact, want), f"{name} {e}: {np.count_nonzero(exact != want)} of {d2.size} exact-form values differ"
        dev = float(np.max(np.abs(fast.astype(np.float64) - want)))
        print(f"{name} {e}: fast form deviates by {dev:.3e}")
        if dev > worst[0]:
            worst = (dev, (name, e))
    assert worst[0] <= BOUND, worst


def test_inlier_census_of_the_fitted_mixtures(fits):
    """countInliers after set_em of those mixtures equals the oracle's on the same coordinates (a non-finite mixture is
    replaced by the default one on both sides)."""
    pairs, g, cases, r = fits["_contexts"][10000]
    ref = OracleGroup(pairs.model, _abi.FrogOptions.default())
    ref.setup_stats()
    xyz2 = g.points()[1]
    ref.set_xyz2(xyz2)
    for i in range(pairs.n_images):
        e = r["warm"][i] if np.all(np.isfinite(r["warm"][i])) else np.float32(er.DEFAULT)
        g.set_em(i, e); ref.set_em(i, e)
    cnt = g.countInliers()
    rcnt = ref.count_inliers((_abi.FrogCounts * pairs.n_images)())
    for i in range(pairs.n_images):
        assert (cnt[i].pairs, cnt[i].inliers, cnt[i].outliers) == (rcnt[i].pairs, rcnt[i].inliers, rcnt[i].outliers), \
            (cases[i // 2]["name"], i, r["warm"][i])
