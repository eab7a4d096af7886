"""Stats::estimateDistribution (stats.cxx:14-70) restated in NumPy / plain Python, one term at a time, and a census of
what happens along the four accumulator chains -- what em_scan_kernel's prefix-sum argument (k_stats.hip.h) hands to
the real arithmetic.  Needs no device.

    membership   f32 c * x^2, f64 exp (libm's, through math.exp), f32 f1, f64 f2 rounded to f32, the `+ 1e-16`
    sum1, sum2   s = fl32(s + v)               v = t * p, t            (f32 terms)
    sum3, sum4   s = fl32(fl64(s + v))         v = (1.0 - t) * p, (1.0 - t)   (f64 terms)
    then the clamps and the stop test.

The census is taken on those sequential sums, never on the kernel's integers: for the step s -> s' with term v,
    special   s is zero, denormal or non-finite
    exit      s is normal and s' has another exponent
    tie       s is normal and v / ulp(s) has fraction exactly 1/2 (split by the parity of s' last bit, and by the way it went)
    near      the fraction is within 2^-20 of 1/2, not equal
and a batch of 64 consecutive terms is `clean` when it holds none of them.

The second half of the file builds the case families tests/test_em_restate.py and tests/test_gpu_em_edges.py share."""
import math

import numpy as np

F4, F8 = np.float32, np.float64
ESP = F4(1.59576912160573)
C0 = F4(0.797884560802865)
ACCUMULATORS = ("sum1", "sum2", "sum3", "sum4")
NEAR = 2.0 ** -20


def chi_pdf(x):
    """stats.h:10-16 for an f32 array: f32 x*x and c*x2, the exponential and the product in f64, rounded to f32."""
    x2 = x * x
    cx2 = C0 * x2
    e = np.array([math.exp(a) for a in (-0.5 * x2.astype(F8)).tolist()], F8)
    assert x2.dtype == cx2.dtype == F4
    return (cx2.astype(F8) * e).astype(F4)


def membership(smp, c1, c2, ratio):
    c1, c2, ratio = F4(c1), F4(c2), F4(ratio)
    f1 = ratio * chi_pdf(smp / c1) / c1
    f2 = ((1.0 - float(ratio)) * chi_pdf(smp / c2).astype(F8) / float(c2)).astype(F4)
    t = (f1.astype(F8) / ((f1 + f2).astype(F8) + 1e-16)).astype(F4)
    assert f1.dtype == f2.dtype == F4
    return t


def chain_f32(v):
    """s = fl32(s + v_k) from s = 0: every prefix (ufunc.accumulate adds strictly in order)."""
    return np.add.accumulate(v, dtype=F4) if len(v) else np.zeros(0, F4)


def chain_f64(v):
    """s = fl32(fl64(s + v_k)) from s = 0: every prefix."""
    out, s = [], 0.0
    for x in v.tolist():
        s = float(F4(s + x))
        out.append(s)
    return np.array(out, F4)


def census(sums, v):
    """sums[k]: the f32 sum after term k; v[k]: term k (f64; an f32 term converts exactly)."""
    n = len(v)
    before = np.concatenate([np.zeros(1, F4), sums[:-1]]) if n else np.zeros(0, F4)
    bb, ba = before.view(np.uint32), np.ascontiguousarray(sums).view(np.uint32)
    exb, exa = (bb >> 23) & 0xFF, (ba >> 23) & 0xFF
    special = (exb == 0) | (exb == 255)
    normal = ~special
    e = exb.astype(np.int64) - 127
    x = np.ldexp(np.where(normal & np.isfinite(v), v, 0.0), np.where(normal, 23 - e, 0))      # v / ulp(s), exact
    frac = x - np.floor(x)
    tie = normal & (frac == 0.5)
    near = normal & (np.abs(frac - 0.5) < NEAR) & ~tie
    exits = normal & (exa != exb)
    odd = (bb & 1) == 1
    went_up = (sums.astype(F8) - before.astype(F8)) > v
    any_event = special | exits | tie | near
    nb = (n + 63) // 64
    dirty = np.zeros(nb, bool)
    np.logical_or.at(dirty, np.arange(n) // 64, any_event)
    return {"n": n, "special": int(special.sum()), "exit": int(exits.sum()), "exit_at": np.nonzero(exits)[0],
            "exit_exact": int((exits & ((ba & 0x7FFFFF) == 0)).sum()),         # the sum lands on the power of two itself
            "tie": int(tie.sum()), "tie_even": int((tie & ~odd).sum()), "tie_odd": int((tie & odd).sum()),
            "tie_up": int((tie & went_up).sum()), "tie_down": int((tie & ~went_up).sum()),
            "near": int(near.sum()), "frac": frac, "normal": normal,
            "batches": nb, "clean_batches": int((~dirty).sum()), "denormal": int(((exb == 0) & (bb != 0)).sum()),
            "zero": int((bb == 0).sum()), "nonfinite": int((exb == 255).sum()), "term_nonfinite": int((~np.isfinite(v)).sum()),
            "ends_nonfinite": int(n > 0 and not np.isfinite(sums[-1]))}


def estimate(samples, start=(10.0, 300.0, 0.5), max_iterations=10000, epsilon=1e-6, census_at=()):
    """(params f32[3], iterations run, {iteration: {accumulator: census, "t": memberships}}) -- iterations count from 1."""
    smp = np.ascontiguousarray(samples, F4)
    n = len(smp)
    c1, c2, ratio = (F4(a) for a in start)
    eps = F4(epsilon)
    found = {}
    iteration = 0
    with np.errstate(all="ignore"):
        while iteration < max_iterations:
            iteration += 1
            t = membership(smp, c1, c2, ratio)
            p = smp * F4(1)                                  # weights are all 1 (addSample's default)
            one_minus_t = 1.0 - t.astype(F8)
            terms = (t * p, t, one_minus_t * p.astype(F8), one_minus_t * 1.0)
            chains = (chain_f32(terms[0]), chain_f32(terms[1]), chain_f64(terms[2]), chain_f64(terms[3]))
            if iteration in census_at:
                found[iteration] = {a: census(chains[k], terms[k].astype(F8)) for k, a in enumerate(ACCUMULATORS)}
                found[iteration]["t"] = t
            sum1, sum2, sum3, sum4 = (c[-1] if n else F4(0) for c in chains)
            sum5 = F4(n)                                     # n additions of 1.0f, exact below 2^24
            # std::max(a, b) is (a < b) ? b : a -- a NaN first argument stays, a NaN second argument is dropped
            cmax = lambda a, b: b if a < b else a
            sum2 = cmax(sum2, eps); sum3 = cmax(sum3, eps); sum5 = cmax(sum5, eps)      # sum4 is not floored (stats.cxx:42-44)
            nc1 = cmax(eps, sum1 / sum2 / ESP)
            nc2 = cmax(eps, sum3 / sum4 / ESP)
            nr = cmax(eps, sum2 / sum5)
            assert all(type(a) is F4 for a in (nc1, nc2, nr))
            done = (float(abs((c1 - nc1) / nc1)) < 0.001 and float(abs((c2 - nc2) / nc2)) < 0.001
                    and float(abs((nr - ratio) / nr)) < 0.001)
            c1, c2, ratio = nc1, nc2, nr
            if done:
                break
    return np.array([c1, c2, ratio], F4), iteration, found


# ---- the case families ------------------------------------------------------------------------------------------------------
# A case: name, samples (f32, in the order the fit walks them), start parameters, iteration cap, and `wants`: what its census
# must show -- (accumulator, census key, least count) in the first EM iteration, `later`: the same in iteration 2.
# T0 / T1: start parameters under which every membership is exactly 0 / exactly 1, so that the terms of sum3 / sum1 are the
# samples themselves and those of sum4 / sum2 are 1.0:
#   T0  c1 = 1e-10: x / c1 >= 1e9 x, exp(-x^2 / 2 c1^2) underflows to 0 in f64 for every x >= 2^-23, f1 = 0, t = 0 / (..) = 0;
#       after the first iteration c1 = ratio = epsilon and f1 is still 0 for every x >= 2^-10: the second iteration repeats
#       the first one's sums (with the guesses the first one left) and the fit stops there.
#   T1  ratio = 1: f2 = 0 * .. = 0, and t = f1 / (f1 + 1e-16) rounds to 1.0f once f1 > 2^25 1e-16 = 3.4e-9, which
#       c1 = 2^-9 gives for 6e-9 < x < 1.3e-2.  sum4 stays 0, so c2 = epsilon / 0 = inf and the fit cannot meet its stop test:
#       these cases run under an iteration cap -- 1 where the first iteration's sum1 has to BE the result (c1 = sum1 / n / esp:
#       later iterations, whose memberships are ordinary, end in the clamp c1 = epsilon whatever sum1 was), 6 elsewhere.
T0 = (1e-10, 300.0, 0.5)
T1 = (2.0 ** -9, 300.0, 1.0)
DEFAULT = (10.0, 300.0, 0.5)
COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 8191, 8192, 8193, 16385, 65537, 70001)


def two_scale(n, seed):
    """Ordinary distances: 60 % inliers of a few mm, 40 % outliers of tens of mm (three-dimensional Gaussian norms)."""
    rng = np.random.default_rng(seed)
    sigma = np.where(rng.random(n) < 0.6, 4.0, 70.0)
    return (np.linalg.norm(rng.normal(size=(n, 3)), axis=1) * sigma).astype(F4)


def _case(name, samples, start=DEFAULT, cap=10000, wants=(), later=()):
    smp = np.asarray(samples, F4)
    return {"name": name, "samples": smp, "coordinates": smp, "start": tuple(float(F4(a)) for a in start), "cap": cap,
            "wants": tuple(wants), "later": tuple(later)}


def _steer(n, jumps, first, unit=1.0):
    """n samples that are `unit` each, except sample 0 = first and sample i = whatever takes the running sum to jumps[i]
    (all in multiples of `unit`, all sums exact)."""
    out, s = [], 0
    for i in range(n):
        v = first if i == 0 else (jumps[i] - s if i in jumps else 1)
        assert v >= 0
        s += v
        out.append(v * unit)
    assert s < 2 ** 24
    return np.array(out, F4)


def _tie_terms(rng, n):
    """Multiples of 1/4 for a sum whose ulp is 1: halves (ties), whole numbers (they flip the parity of S) and quarters."""
    return rng.choice([0.5, 1.5, 2.5, 1.0, 3.0, 0.25, 0.75, 0.5, 1.5], n)


def count_cases():
    out = []
    for k, n in enumerate(COUNTS):
        # what a count is for: the step from the zero sum (every count; the partial last batch follows from the count itself);
        # batches the kernel may take the short way, in the second iteration, next to the chunk edges (from 8 191 on);
        # batches past the 1 024 that keep a guess (from 65 537 on)
        wants = [("sum1", "special", 1), ("sum3", "special", 1)]
        later = [(a, "clean_batches", 64) for a in ACCUMULATORS] if n >= 8191 else []
        if n > 65536:
            later += [(a, "batches", 1025) for a in ACCUMULATORS]
        out.append(_case(f"count_{n}", two_scale(n, 100 + k), wants=wants, later=later))
    # the same counts with every membership 0: sum4 is the count itself, leaves a binade at every power of two (lane 63 of a
    # batch from 64 on) and lands on the power exactly -- S + T = 2^24 for the batch 64 -> 128 in the second iteration
    for n in (129, 8193, 65537):
        ex = int(math.log2(n))
        out.append(_case(f"count_{n}_t0", two_scale(n, 200 + n) + F4(1), T0, wants=[("sum4", "exit_exact", min(ex, 8))],
                         later=[("sum4", "exit_exact", min(ex, 8))]))
    return out


def tie_cases():
    rng = np.random.default_rng(7)
    small = _tie_terms(rng, 448)
    # 64 x 2^17 lift the sum to 2^23 (ulp 1); from there halves are exact ties
    s3 = np.concatenate([np.full(64, 2.0 ** 17), small])
    w3 = [("sum3", "tie_even", 8), ("sum3", "tie_odd", 8), ("sum3", "tie_up", 8), ("sum3", "tie_down", 8)]
    # the same pattern 2^-24 times as large: 64 x 2^-7 lift the sum to 1/2 (ulp 2^-24), inside T1's range of samples
    s1 = (s3 * 2.0 ** -24).astype(F4)
    w1 = [("sum1", "tie_even", 8), ("sum1", "tie_odd", 8), ("sum1", "tie_up", 8), ("sum1", "tie_down", 8)]
    # sum4 / sum2 = the count: 1.0 meets a sum of ulp 2 from 2^24 on, which no image reaches; their ties are out of range
    w1.append(("sum4", "zero", len(s1)))            # every membership is 1: sum4 never leaves 0
    return [_case("ties_sum3", s3, T0, wants=w3, later=w3), _case("ties_sum1", s1, T1, cap=1, wants=w1)]


def near_tie_cases():
    rng = np.random.default_rng(8)
    inside = [k + 0.5 + s * 2.0 ** -b for k, bs in ((0, (21, 22, 23)), (1, (21, 22, 23)), (2, (21, 22)), (3, (21, 22)))
              for b in bs for s in (1, -1)]
    outside = [k + 0.5 + s * 2.0 ** -19 for k in range(8) for s in (1, -1)]
    body = np.concatenate([rng.permutation(inside * 6), rng.permutation(outside * 6), rng.permutation(inside * 2 + outside * 2)])
    assert np.array_equal(body.astype(F4).astype(F8), body)
    s = np.concatenate([np.full(64, 2.0 ** 17), body])
    # With every membership 0 the terms are f32 values and the f64 add S + v is exact: the two roundings of the reference
    # and the single one of the integer form agree with or without the window.  What the family holds is that a term inside
    # the window comes out right through the real arithmetic and one just outside it through the integer rounding; it cannot
    # tell how wide the window has to be (that needs an f64 product within 2^-29 of a tie, which no choice of samples forces).
    w = [("sum3", "near", 8), ("sum3", "outside_window", 8)]
    return [_case("near_ties_sum3", s, T0, wants=w, later=w)]


def exit_cases():
    out = []
    # sums in whole numbers, all exact: what is exercised is where the sum leaves its binade, not the rounding
    lane0 = _steer(64 * 10, {64 * b: 2 ** (9 + b) + 3 for b in range(1, 10)}, 600)
    lane63 = _steer(64 * 10, {64 * b + 63: 2 ** (10 + b) + 3 for b in range(0, 10)}, 600)
    twice = _steer(64 * 10, {**{64 * b + 10: 2 ** (5 + 2 * b) + 3 for b in range(1, 9)},
                             **{64 * b + 40: 2 ** (6 + 2 * b) + 3 for b in range(1, 9)}}, 3)
    # the sum after lane 63 is the power of two itself: the next batch starts at the bottom of a new binade
    between = _steer(64 * 10, {64 * b + 63: 2 ** (10 + b) for b in range(0, 10)}, 600)
    for name, s, key in (("exit_lane0", lane0, "exit_lane0"), ("exit_lane63", lane63, "exit_lane63"),
                         ("exit_twice", twice, "exit_twice"), ("exit_between_batches", between, "exit_between")):
        w = [("sum3", key, 8)]
        out.append(_case(name, s, T0, wants=w, later=w))
    # batch A_k: the sum goes from 2^k to 2^(k+1) - ulp, S + T = 2^24 - 1; batch B_k: one ulp more, S + T = 2^24 exactly, then zeros
    s, k = [2.0 ** 20], 20
    s += [0.0] * 63
    for rep in range(8):
        u = 2.0 ** (k - 23)
        s += [131072 * u] * 63 + [(2 ** 23 - 1 - 63 * 131072) * u]
        s += [u] + [0.0] * 63
        k += 1
    w = [("sum3", "batch_ends_one_below", 8), ("sum3", "exit_exact", 8)]
    out.append(_case("exit_one_unit", np.array(s), T0, wants=w, later=w))
    return out


def zero_cases():
    out = [_case("zeros_default", np.zeros(200), DEFAULT, wants=[("sum1", "zero", 200), ("sum3", "zero", 200)],
                 later=[("sum3", "zero", 200)]),
           _case("zeros_t0", np.zeros(200), T0, wants=[("sum3", "zero", 200)], later=[("sum3", "zero", 200)])]
    for name, at in (("zeros_then_lane0", 64), ("zeros_then_lane63", 127), ("zeros_then_later_batch", 300)):
        s = np.zeros(400)
        s[at:] = two_scale(400 - at, at) + F4(1)
        out.append(_case(name, s, T0, wants=[("sum3", "zero", at + 1)], later=[("sum3", "zero", at + 1)]))
        s1 = np.zeros(400)
        s1[at:] = (two_scale(400 - at, at) + F4(1)) * F4(2.0 ** -16)
        out.append(_case(name + "_t1", s1, T1, cap=6, wants=[("sum1", "zero", at + 1), ("sum2", "zero", at + 1)]))
    # coordinates of 1e-41 .. 1e-38: the f32 squared distance underflows to 0, so the retained samples ARE 0 -- no distance
    # below sqrt(2^-149) = 3.7e-23 other than 0 can be retained; the fit sees an all-zero image
    c = _case("denormal_coordinates", np.zeros(200), DEFAULT, wants=[("sum1", "zero", 200)])
    c["coordinates"] = np.geomspace(1e-41, 1e-38, 200).astype(F4)
    out.append(c)
    # what a fit can meet instead: denormal TERMS.  x / c1 from 14.4 down to 13.0 puts f1 between 1e-43 and 1e-35 while
    # f2 = 0.03: the memberships t (sum2) and t * x (sum1) are denormal first and normal later, and so are the sums
    rho = np.concatenate([np.linspace(14.4, 13.9, 100), np.linspace(13.9, 13.0, 92)])
    out.append(_case("denormal_terms", rho, (1.0, 10.0, 0.5), wants=[("sum1", "denormal", 8), ("sum2", "denormal", 8),
                                                                         ("sum1", "left_denormal_mid_batch", 1),
                                                                         ("sum2", "left_denormal_mid_batch", 1)]))
    return out


def nonfinite_cases():
    out = []
    for name, at in (("inf_first", 0), ("inf_middle", 100), ("inf_last", 199)):
        s = two_scale(200, 300 + at)
        coords = s.copy()
        coords[at] = 1e20                                   # the f32 squared distance overflows: the sample is inf
        s[at] = np.inf
        # one non-finite sample (as the family is set): its term is NaN in every chain and so is the sum at the end; where
        # it is not the last sample, every later step is taken with a non-finite sum -- 199 - at of them
        c = _case(name, s, DEFAULT, wants=[(a, "term_nonfinite", 1) for a in ACCUMULATORS]
                  + [(a, "nonfinite", 199 - at) for a in ACCUMULATORS if at < 199] + [(a, "ends_nonfinite", 1) for a in ACCUMULATORS])
        c["coordinates"] = coords
        out.append(c)
    return out


def all_cases():
    return count_cases() + tie_cases() + near_tie_cases() + exit_cases() + zero_cases() + nonfinite_cases()


def derived(cen):
    """The census keys of `wants` that are not plain counts of census()."""
    at = cen["exit_at"]
    lanes = at % 64
    per_batch = np.bincount(at // 64, minlength=cen["batches"]) if len(at) else np.zeros(cen["batches"], int)
    d = dict(cen)
    d["exit_lane0"] = int((lanes == 0).sum())
    d["exit_lane63"] = int((lanes == 63).sum())
    d["exit_twice"] = int((per_batch >= 2).sum())
    d["outside_window"] = int((cen["normal"] & (np.abs(np.abs(cen["frac"] - 0.5) - 2.0 ** -19) == 0)).sum())
    return d


def check_wants(case, found, which="wants", iteration=1):
    """Assert that the census of `iteration` shows what the case is for."""
    chains = None
    for acc, key, least in case[which]:
        d = derived(found[iteration][acc])
        if key in ("exit_between", "batch_ends_one_below", "left_denormal_mid_batch"):
            if chains is None:
                chains = _prefixes(case, found[iteration]["t"])
            sums = chains[acc]
            bits = sums.view(np.uint32)
            ends = np.arange(63, len(sums), 64)
            if key == "exit_between":           # the sum after lane 63 is a power of two it was below at lane 62
                got = int(((bits[ends] & 0x7FFFFF) == 0).sum())
            elif key == "batch_ends_one_below":  # the sum after lane 63 is one unit below a power of two, and the batch began in that binade
                starts = ends - 64
                ok = ((bits[ends] & 0x7FFFFF) == 0x7FFFFF) & (starts >= 0)
                got = int((ok & ((bits[np.maximum(starts, 0)] >> 23) == (bits[ends] >> 23))).sum())
            else:                               # a denormal sum becomes normal at a lane other than 0
                ex = (bits >> 23) & 0xFF
                k = np.nonzero((ex[1:] != 0) & (ex[:-1] == 0) & (bits[:-1] != 0))[0] + 1
                got = int(((k % 64) != 0).sum())
        else:
            got = d[key]
        assert got >= least, f"{case['name']}: {acc} {key} = {got} in iteration {iteration}, at least {least} wanted"


def _prefixes(case, t):
    p = case["samples"]
    with np.errstate(all="ignore"):
        omt = 1.0 - t.astype(F8)
        return {"sum1": chain_f32(t * p), "sum2": chain_f32(t), "sum3": chain_f64(omt * p.astype(F8)), "sum4": chain_f64(omt)}


# ---- what the two test modules share ----------------------------------------------------------------------------------------

def oracle_fit(which, samples, start, cap):
    """Stats("oracle") or Stats("ref") on `samples` from `start` under the iteration cap: (c1, c2, ratio)."""
    from oracle.oracle_api import Stats
    s = Stats(which, max_size=max(len(samples), 1), max_iterations=cap)
    s.add_slots(len(samples))
    s.set_params(np.asarray(start, F4))
    s.reset(); s.add_samples(np.asarray(samples, F4)); s.estimate()
    return s.params()


def same(a, b):
    """Bit for bit; a non-finite component by its class (NaN, +inf, -inf), not its payload."""
    a, b = np.asarray(a, F4), np.asarray(b, F4)
    fin = np.isfinite(a) & np.isfinite(b)
    return bool(np.array_equal(a[fin], b[fin]) and np.array_equal(np.isnan(a), np.isnan(b))
                and np.array_equal(np.isinf(a) * np.sign(a), np.isinf(b) * np.sign(b)))
