"""The arguments behind the culling list's certificate (k_cull.hip.h), checked on its numpy restatement (tests/cull_restate.py):
the displacement a list allows is sound in exact arithmetic, and the probability the cutoff is placed on does not come back
up behind it."""
import numpy as np

import cull_restate as cr

F = np.float32
THRESHOLDS = (0.5, 0.1, 0.99, 1e-3)


def random_mixture(rng):
    """The generator of tests/test_gpu_round2.py::test_inlier_weight_pair_random_mixtures, with c2 > c1."""
    c1 = float(F(10.0 ** rng.uniform(-2, 2)))
    c2 = float(F(c1 * 10.0 ** rng.uniform(0.001, 3)))
    r = float(F(rng.choice([rng.uniform(0.01, 0.99), 10.0 ** rng.uniform(-6, -2), 1 - 10.0 ** rng.uniform(-6, -2)])))
    return (c1, c2, r)


def mixtures(n, seed):
    rng = np.random.default_rng(seed)
    out = [random_mixture(rng) for _ in range(n)]
    for c1 in (0.05, 3.0, 70.0):                    # c1 close to c2, ratios at the ends
        for q in (1.0 + 2.0 ** -20, 1.001, 1.1):
            out.append((c1, float(F(c1 * q)), 0.5))
        out += [(c1, 50.0 * c1, 1e-6), (c1, 50.0 * c1, 1.0 - 1e-6)]
    return out


def test_allowance_is_sound_in_exact_arithmetic():
    """Whenever the check passes at displacement D -- cull_validate_kernel's f32 condition, or D <= cull_allow_kernel's f32
    allowance, which is what the transforms compare with -- cut_list[k] - 2 D >= cut_now[k] holds in f64 for every image."""
    rng = np.random.default_rng(17)
    n_fresh = n_stale = n_at_allow = 0
    for trial in range(400):
        nI = int(rng.integers(1, 40))
        thr = THRESHOLDS[trial % len(THRESHOLDS)]
        now = np.array([cr.cull_cutoff_of(random_mixture(rng), thr) for _ in range(nI)], F)
        if trial % 3 == 0:
            now = (10.0 ** rng.uniform(-0.7, 4.0, nI)).astype(F)            # cutoffs of any size, not only a mixture's
        if trial % 5 == 0:
            now[rng.integers(0, nI)] = np.inf                               # an image without a cutoff
        scale, pad = float(rng.choice([1.0, 1.05, 1.2, 2.0])), float(rng.choice([0.0, 0.5, 1.0, 3.0, 25.0]))
        lst = cr.list_cutoff(now, scale, pad)
        allow = cr.allowance(now, lst)
        exact = lambda D: np.all(lst.astype(np.float64) - 2.0 * float(D) >= now.astype(np.float64))
        finite = np.isfinite(now)
        if allow == allow and allow >= 0 and finite.any():
            # the allowance itself, the floats around it, and displacements spread around it
            for D in [allow, np.nextafter(allow, F(0)), np.nextafter(allow, F(np.inf))] + list((allow * rng.uniform(0.0, 2.0, 6)).astype(F)):
                D = F(D)
                st = cr.stale(now, lst, D)
                if D <= allow:
                    n_at_allow += 1
                    assert exact(D), (now, lst, D, allow)
                if not st:
                    n_fresh += 1
                    assert exact(D), (now, lst, D, allow)
                else:
                    n_stale += 1
        else:
            # no room at all (a zero skin): already D = 0 is stale, or the statement holds
            if not cr.stale(now, lst, F(0)):
                n_fresh += 1
                assert exact(0.0)
            else:
                n_stale += 1
        assert cr.stale(now, lst, F(np.nan))
    assert n_fresh >= 200 and n_stale >= 200 and n_at_allow >= 200, (n_fresh, n_stale, n_at_allow)


def test_allowance_and_check_agree_on_what_they_let_pass():
    """A displacement the transforms let pass (D <= allowance) is one the stand-alone check lets pass too: the flag a transform
    leaves down is not one the check would have raised."""
    rng = np.random.default_rng(23)
    n = 0
    for trial in range(300):
        nI = int(rng.integers(1, 40))
        now = (10.0 ** rng.uniform(-0.7, 3.0, nI)).astype(F)
        lst = cr.list_cutoff(now, float(rng.choice([1.0, 1.05, 2.0])), float(rng.choice([0.5, 1.0, 2.0, 25.0])))
        allow = cr.allowance(now, lst)
        if allow >= 0:
            n += 1
            assert not cr.stale(now, lst, allow), (now, lst, allow)
    assert n >= 200


def test_probability_does_not_come_back_up_behind_the_cutoff():
    """mixture_probability at the restated cutoff is at most threshold / 2 and non-increasing from there to 1e3 cutoffs.
    Non-increasing is a statement about the f64 values while the exponential is a normal number: once exp(-a^2 / 2) is
    denormal it has fewer than 53 bits and stays put over a stretch in which its factor a^2 still grows, so the product can
    step up in its last bits (seen: 3.433e-309 -> 3.436e-309).  There x1 < 1e-290 and p = x1 / (x1 + x2 + 1e-10) < 1e-280:
    below 1e-280 the test asks that p stays below 1e-280, everywhere else that it does not rise at all."""
    n = 0
    for k, em in enumerate(mixtures(240, 31)):
        thr = THRESHOLDS[k % len(THRESHOLDS)]
        cut = cr.cull_cutoff_of(em, thr)
        assert np.isfinite(cut), (em, thr)              # c1 < c2, ratio inside (0, 1): the search ends
        em32 = tuple(float(F(v)) for v in em)
        d = np.geomspace(float(cut), 1e3 * float(cut), 10000)
        p = cr.mixture_probability(d, *em32)
        assert p[0] <= 0.5 * float(F(thr)), (em, thr, cut, p[0])
        tiny = p[:-1] < 1e-280
        assert np.all((np.diff(p) <= 0.0) | tiny), (em, thr, cut)
        assert np.all(p[1:][tiny] < 1e-280), (em, thr, cut)
        n += 1
    assert n >= 200


def test_degenerate_mixtures_have_no_cutoff():
    for em in [(5.0, 3.0, 0.5), (3.0, 3.0, 0.5), (3.0, 200.0, 0.0), (3.0, 200.0, 1.0), (3.0, 200.0, -0.1), (3.0, 200.0, 1.5),
               (3.0, 200.0, np.nan), (0.0, 200.0, 0.5), (3.0, np.inf, 0.5), (3.0, 1e30, 0.5), (np.nan, 200.0, 0.5)]:
        assert cr.cull_cutoff_of(em, 0.5) == np.inf, em
    assert cr.cull_cutoff_of((3.0, 200.0, 0.7), 9e-4) == np.inf
    assert np.isfinite(cr.cull_cutoff_of((3.0, 200.0, 0.7), 1e-3))


def test_list_rule_at_its_edges():
    cut = F(37.25)
    c2 = F(cut * cut)
    d2 = np.array([np.nextafter(c2, F(0)), c2, np.nextafter(c2, F(np.inf)), np.nan, np.inf, 0.0], F)
    assert cr.listed(d2, cut, F(80.0)).tolist() == [True, False, False, True, True, True]
    assert cr.listed(d2, F(80.0), cut).tolist() == [True, False, False, True, True, True]
    assert cr.listed(d2, cut, F(np.inf)).tolist() == [True, False, False, True, True, True]
    assert cr.listed(d2, F(np.inf), F(np.inf)).all()            # no cutoff: everything is listed
    x = np.array([[0, 0, 0], [3, 4, 12], [np.nan, 0, 0]], F)
    assert cr.link_d2(x, [0, 0], [1, 2])[0] == 169.0 and np.isnan(cr.link_d2(x, [0, 0], [1, 2])[1])
