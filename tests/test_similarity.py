"""similarity_fit (frog_amd/csrc/device/similarity.h) by itself, through tests/similarity_driver.cpp: the fit of the RANSAC
stage's candidates and of its refit.

Accepted fits are compared with Horn's closed form at 60 digits (mpmath) and with Kabsch through numpy's SVD.  The bound is
K * 2^-52 * magnitude / relgap (tests/similarity_util.py: error_bound).  K: the SVD solution's worst ratio to that bound with
K = 1 over the cases below is 4.7 (`python tests/test_similarity.py` prints the ratios), taken as 5; similarity_fit is allowed
four times that, K = 20: both are backward-stable float64 solvers of the same problem, the factor covers the order of their
operations.  similarity_fit's own ratios were not used to choose K.

Undetermined rotations must be refused.  In exact arithmetic they have l1 == l2 (the two largest eigenvalues of N); in float64
the two end up a few ulps apart, and the exact comparison similarity_fit made before it compared against
SIMILARITY_MIN_RELATIVE_GAP let about 85 % of the exactly degenerate four-point draws through.
`python tests/test_similarity.py 100000` is the measurement behind that constant."""
import math
import sys

import numpy as np
import pytest

import similarity_util as su
from similarity_util import F4, F8, EPS, K, K_SVD

KINDS_DEGENERATE = ("two_twice", "three_one", "collinear")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = su.build_driver(tmp_path_factory.mktemp("similarity"))
    if exe is None:
        pytest.skip("no C++ compiler")
    return exe


# ---- the accepted cases ---------------------------------------------------------------------------------------------------
def rotation(rng):
    q = rng.normal(size=4)
    return quaternion_matrix(q / np.linalg.norm(q))


def quaternion_matrix(q):
    w, x, y, z = q
    return np.array([[w*w + x*x - y*y - z*z, 2 * (x*y - w*z), 2 * (x*z + w*y)],
                     [2 * (x*y + w*z), w*w - x*x + y*y - z*z, 2 * (y*z - w*x)],
                     [2 * (x*z - w*y), 2 * (y*z + w*x), w*w - x*x - y*y + z*z]])


def moved(a, R, s, t, rng=None, noise=0.0):
    b = s * a @ R.T + t
    return b + rng.normal(0, noise, b.shape) if noise else b


def accepted_cases():
    """name -> (source, target), float32; every one has a determined rotation."""
    rng = np.random.default_rng(20)
    cases = {}
    for n in (3, 4, 50, 5000):
        a = rng.uniform(-100, 100, (n, 3))
        R, t = rotation(rng), rng.uniform(-50, 50, 3)
        cases[f"generic_{n}_clean"] = (a, moved(a, R, 1.25, t))
        cases[f"generic_{n}_noise"] = (a, moved(a, R, 1.25, t, rng, 2.0))
    for n in (4, 50):
        a = rng.uniform(-100, 100, (n, 3))
        cases[f"mirror_{n}"] = (a, moved(a, rotation(rng), 0.8, rng.uniform(-50, 50, 3)) * np.array([1.0, 1.0, -1.0]))
        flat = a * np.array([1.0, 1.0, 0.0])
        cases[f"coplanar_{n}"] = (flat, moved(flat, rotation(rng), 1.1, rng.uniform(-50, 50, 3)))
    a = 1e4 + rng.uniform(-1e-2, 1e-2, (50, 3))
    cases["far_centroid_small_spread"] = (a, 1e4 + (a.astype(F4).astype(F8) - 1e4) @ rotation(rng).T)
    for e in range(-3, 4):
        a = rng.uniform(-100, 100, (10, 3))
        cases[f"scale_1e{e}"] = (a, moved(a, rotation(rng), 10.0 ** e, rng.uniform(-50, 50, 3)))
    for name, axis in (("x", (1, 0, 0)), ("y", (0, 1, 0)), ("z", (0, 0, 1)), ("oblique", (1, 2, -2))):
        a = rng.uniform(-100, 100, (10, 3))
        q = np.array((0.0,) + axis, F8)
        cases[f"half_turn_{name}"] = (a, moved(a, quaternion_matrix(q / np.linalg.norm(q)), 1.0, rng.uniform(-50, 50, 3)))
    return {k: (np.asarray(a, F4), np.asarray(b, F4)) for k, (a, b) in cases.items()}


CASES = accepted_cases()


@pytest.fixture(scope="module")
def fitted(driver):
    names = sorted(CASES)
    ok, out, top2 = su.run_driver(driver, [CASES[k] for k in names])
    return {k: (ok[i], out[i], top2[i]) for i, k in enumerate(names)}


@pytest.fixture(scope="module")
def reference():
    pytest.importorskip("mpmath")
    return {k: su.horn_mp(a, b) for k, (a, b) in CASES.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_fit_matches_the_60_digit_reference(fitted, reference, name):
    ok, out, top2 = fitted[name]
    ref, relgap, mag = reference[name]
    assert ok
    err, bound = su.max_error(out, ref), su.error_bound(relgap, mag)
    print(f"{name}: error {err:.3e}, bound {bound:.3e}, ratio to K = 1: {err / su.error_bound(relgap, mag, 1.0):.3f}")
    assert err <= bound
    # the eigenvalues the decision is taken on are N's
    assert (top2[0] - top2[1]) / abs(top2[0]) == pytest.approx(relgap, rel=1e-6, abs=1e-9)


@pytest.mark.parametrize("name", sorted(CASES))
def test_svd_reference_is_within_a_quarter_of_K(reference, name):
    """The measurement K comes from, kept in place: numpy's SVD solution against the 60-digit one."""
    ref, relgap, mag = reference[name]
    assert su.max_error(su.kabsch_svd(*CASES[name]), ref) <= su.error_bound(relgap, mag, K_SVD)


@pytest.mark.parametrize("name", sorted(CASES))
def test_fit_matches_the_svd_solution(fitted, name):
    """Runs without mpmath too: both solutions are within their bounds of the truth, so within the sum of each other."""
    ok, out, _ = fitted[name]
    relgap, mag = su.relgap_f64(*CASES[name])
    assert ok
    assert np.abs(out - su.kabsch_svd(*CASES[name])).max() <= su.error_bound(relgap, mag, K + K_SVD)


@pytest.mark.parametrize("name", sorted(CASES))
def test_fit_is_a_proper_similarity_between_the_centroids(fitted, name):
    ok, out, _ = fitted[name]
    a, b = (v.astype(F8) for v in CASES[name])
    m = out[:3, :3]
    s2 = np.trace(m @ m.T) / 3
    assert ok and np.array_equal(out[3], [0, 0, 0, 1])
    assert np.abs(m @ m.T - s2 * np.eye(3)).max() <= K * EPS * s2
    assert np.linalg.det(m) > 0
    ca = np.array([math.fsum(a[:, k]) for k in range(3)]) / len(a)
    cb = np.array([math.fsum(b[:, k]) for k in range(3)]) / len(b)
    assert np.abs(m @ ca + out[:3, 3] - cb).max() <= K * EPS * max(np.sqrt(s2), np.abs(cb).max(), np.sqrt(s2) * np.abs(ca).sum())


def test_mirror_image_gets_the_best_proper_rotation(fitted):
    """Horn's quaternion cannot express a reflection: the answer is the determinant-corrected SVD's, and it does not
    reproduce the target (the residual is the price of det = +1)."""
    for name in ("mirror_4", "mirror_50"):
        ok, out, _ = fitted[name]
        a, b = (v.astype(F8) for v in CASES[name])
        assert ok and np.linalg.det(out[:3, :3]) > 0
        assert np.abs(a @ out[:3, :3].T + out[:3, 3] - b).max() > 1.0
        U, S, Vt = np.linalg.svd((a - a.mean(0)).T @ (b - b.mean(0)))
        assert np.linalg.det(Vt.T @ U.T) < 0                       # the uncorrected optimum is a reflection


def test_half_turns_have_no_real_part(fitted):
    for name in ("half_turn_x", "half_turn_y", "half_turn_z", "half_turn_oblique"):
        m = fitted[name][1][:3, :3]
        assert abs(np.trace(m) + 1.0) < 1e-5                       # trace = 4 w^2 - 1


# ---- 0, 1 and 2 points ----------------------------------------------------------------------------------------------------
def test_zero_one_and_two_points(driver):
    a = np.array([[1.5, -2.25, 3.0], [4.0, 0.5, -7.0]], F4)
    b = np.array([[10.0, 20.0, -30.5], [-3.0, 8.0, 1.0]], F4)
    ok, out, _ = su.run_driver(driver, [(a[:0], b[:0]), (a[:1], b[:1]), (a, b), (a[[0, 0]], b[[0, 0]])])
    assert ok[0] and np.array_equal(out[0], np.eye(4))
    shift = np.eye(4)
    shift[:3, 3] = b[0].astype(F8) - a[0].astype(F8)
    assert ok[1] and np.array_equal(out[1], shift)
    assert not ok[2] and np.array_equal(out[2], np.eye(4))
    assert not ok[3] and np.array_equal(out[3], np.eye(4))


# ---- refusals -------------------------------------------------------------------------------------------------------------
def draws(kind, n, offset, rng):
    """n four-point draws, float32 (n, 4, 3) source and target: coordinates in +-100, all moved by 5000 with `offset`.
    two_twice / three_one: two distinct correspondences, drawn 2 + 2 or 3 + 1 times in random order; collinear: four
    sources p + k d with small integers, exact in float32, against generic targets (odd draws: the targets on a line,
    the sources generic); generic: sources and targets independent."""
    a = rng.uniform(-100, 100, (n, 4, 3))
    b = rng.uniform(-100, 100, (n, 4, 3))
    if kind in ("two_twice", "three_one"):
        pick = np.array([0, 1, 0, 1] if kind == "two_twice" else [0, 0, 0, 1])
        idx = rng.permuted(np.tile(pick, (n, 1)), axis=1)[:, :, None]
        a, b = np.take_along_axis(a, idx, 1), np.take_along_axis(b, idx, 1)
    elif kind == "collinear":
        p = rng.integers(-100, 101, (n, 1, 3))
        d = rng.integers(1, 9, (n, 1, 3)) * rng.choice([-1, 1], (n, 1, 3))
        k = rng.permuted(np.tile(np.arange(-6, 7), (n, 1)), axis=1)[:, :4, None]
        line = (p + k * d).astype(F8)
        odd = (np.arange(n) % 2 == 1)[:, None, None]
        a, b = np.where(odd, a, line), np.where(odd, line, b)
    else:
        assert kind == "generic"
    if offset:
        a, b = a + 5000.0, b + 5000.0
    return a.astype(F4), b.astype(F4)


def relative_gaps(driver, kind, n, offset, seed):
    a, b = draws(kind, n, offset, np.random.default_rng(seed))
    ok, out, top2 = su.run_driver(driver, list(zip(a, b)))
    with np.errstate(invalid="ignore", divide="ignore"):
        return ok, out, (top2[:, 0] - top2[:, 1]) / np.abs(top2[:, 0])


@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("kind", KINDS_DEGENERATE)
def test_degenerate_draws_are_refused(driver, kind, offset):
    """Before the relative threshold most of two_twice and three_one came back true, with a rotation about the line that
    rounding had chosen."""
    ok, out, gap = relative_gaps(driver, kind, 2000, offset, 1)
    assert not ok.any(), f"{ok.sum()} of {len(ok)} accepted, largest relative gap {np.nanmax(gap):.2e}"
    assert (out == np.eye(4)).all()


def test_longer_collinear_lists_are_refused(driver):
    rng = np.random.default_rng(2)
    cases = []
    for n in (3, 4, 10, 50, 500):
        k = rng.permutation(np.arange(-300, 301))[:n, None]
        line = (np.array([7, -30, 12]) + k * np.array([3, -1, 2])).astype(F4)
        free = rng.uniform(-100, 100, (n, 3)).astype(F4)
        cases += [(line, free), (free, line), (line, (2 * line + 5).astype(F4))]
    ok, out, _ = su.run_driver(driver, cases)
    assert not ok.any() and (out == np.eye(4)).all()


def test_coincident_sources_or_targets_are_refused(driver):
    rng = np.random.default_rng(3)
    free = rng.uniform(-100, 100, (4, 3)).astype(F4)
    same = np.tile(np.array([[12.5, -40.0, 7.25]], F4), (4, 1))
    ok, out, top2 = su.run_driver(driver, [(same, free), (free, same), (same, same)])      # sa == 0: the scale is x / 0
    assert not ok.any() and (out == np.eye(4)).all() and (top2 == 0).all()


def test_non_finite_input_is_refused(driver):
    a, b = (v[:4].copy() for v in CASES["generic_4_clean"])
    cases = []
    for bad in (np.nan, np.inf):
        for side in (0, 1):
            pair = [a.copy(), b.copy()]
            pair[side][2, 1] = bad
            cases.append(tuple(pair))
    ok, out, _ = su.run_driver(driver, cases)
    assert not ok.any() and (out == np.eye(4)).all()


def test_threshold_lies_between_degenerate_and_generic_gaps(driver):
    """SIMILARITY_MIN_RELATIVE_GAP is a power of two, at least 2^10 above every exactly degenerate draw's gap and at least
    2^10 below every generic draw's (the comment above similarity_fit has the figures of 100 000 draws a kind)."""
    tau = su.tau()
    assert np.log2(tau) == int(np.log2(tau))
    worst = max(np.nanmax(relative_gaps(driver, kind, 2000, offset, 4)[2]) for kind in KINDS_DEGENERATE for offset in (False, True))
    least = min(relative_gaps(driver, "generic", 2000, offset, 4)[2].min() for offset in (False, True))
    print(f"largest degenerate gap {worst:.3e}, tau {tau:.3e}, smallest generic gap {least:.3e}")
    assert worst * 2 ** 10 <= tau and tau * 2 ** 10 <= least
    for offset in (False, True):
        assert relative_gaps(driver, "generic", 2000, offset, 5)[0].all()


# ---- the measurements behind K and the threshold ------------------------------------------------------------------------------
if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        exe = su.build_driver(tmp)
        names = sorted(CASES)
        ok, out, _ = su.run_driver(exe, [CASES[k] for k in names])
        print("ratio of the error to 2^-52 * magnitude / relgap: numpy SVD (K is 4 x its maximum), similarity_fit")
        for i, k in enumerate(names):
            ref, relgap, mag = su.horn_mp(*CASES[k])
            unit = su.error_bound(relgap, mag, 1.0)
            print(f"  {k:28s} relgap {relgap:.3e}  svd {su.max_error(su.kabsch_svd(*CASES[k]), ref) / unit:7.3f}  "
                  f"fit {su.max_error(out[i], ref) / unit:7.3f}")
        n = int(sys.argv[1]) if len(sys.argv) > 1 else 0
        for kind in KINDS_DEGENERATE + ("generic",) if n else ():
            for offset in (False, True):
                ok, _, gap = relative_gaps(exe, kind, n, offset, 6)
                print(f"  {kind:10s} offset {int(offset)}: {n} draws, {int(ok.sum())} accepted, relative gap "
                      f"min {np.nanmin(gap):.3e} max {np.nanmax(gap):.3e}")
