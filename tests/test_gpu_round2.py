"""Round-2 parity work: integer outputs compared with `==`, the sweep's inlier weight pinned on the device
against the reference build of stats.cxx, the ten-case parity sweep with a criterion that does not pick its
cases, certified outlier culling bit-identical to the full sweep, and the layout edge cases the advisor
listed (more than 2048 images, shuffled block order, a context that owns only empty images).
All through the C ABI (include/frog_hip.h)."""
import ctypes as C

import numpy as np
import pytest

from frog_amd import _abi, schedule
from frog_amd.image_group import ImageGroup, device_inlier_probability, device_inlier_weight_pair
from frog_amd.pairs import Pairs
from oracle.oracle_api import OracleGroup, Stats, ref_lib
from gpu_util import _run_schedule, note, relerr

pytestmark = pytest.mark.gpu
REL = 1e-4


# ---- S4 on the device against the reference build ----------------------------------------------------------

MIXTURES = [(c1, c2, r) for c1 in (0.8, 3.0, 10.0, 40.0) for c2 in (60.0, 300.0) for r in (0.05, 0.5, 0.95) if c1 < c2]


def test_inlier_probability_against_the_reference_build():
    """Stats::getInlierProbability (stats.h:84-92).  `exact` (the form with the reference's promotions, which decides
    every weight within 1e-4 of the threshold) must reproduce the reference build bit for bit; `fast` (the f32 form every
    half-link goes through) must stay inside the bound derived in k_links.hip.h (INLIER_PROBABILITY_BOUND = 2^-16)."""
    if ref_lib() is None:
        pytest.fail("oracle/_ref/libfrog_refstats.so (the reference's stats.cxx) was not built")
    bound = 2.0 ** -16
    worst_fast, worst_exact, n_total = 0.0, 0, 0
    rng = np.random.default_rng(4)
    for c1, c2, r in MIXTURES:
        ref = Stats("ref")
        ref.set_params([c1, c2, r])
        # d / c1 over [0.02, 60] (log-spaced), a dense stretch around the inlier threshold crossing, the `d < 0.1`
        # branch and its edge, and random distances
        d = np.concatenate([
            c1 * np.geomspace(0.02, 60.0, 60000),
            np.linspace(0.0, 0.2, 2001),
            np.nextafter(np.float32(0.1), np.float32([0.0, 1.0])),
            rng.uniform(0.0, 5.0 * c2, 40000),
        ]).astype(np.float32)
        want = ref.prob_n(d)
        # where the probability crosses 0.5 (if it does): 20000 consecutive floats around the crossing
        k = int(np.argmin(np.abs(want[:60000] - 0.5)))
        centre = d[k]
        dense = centre + (np.arange(-10000, 10000) * np.spacing(centre)).astype(np.float32)
        d = np.concatenate([d, dense.astype(np.float32)])
        # a sweep step holds d2 (f32) and the reference's `dist` is its correctly rounded f32 square root: feed the
        # device the squares and the reference build the roots of exactly those squares
        d2 = (d * d).astype(np.float32)
        d2 = np.concatenate([d2, np.nextafter(np.float32(0.01), np.float32([0.0, 1.0])), np.float32([0.01])])   # the `d < 0.1` edge in d2
        want = ref.prob_n(np.sqrt(d2))
        fast, exact = device_inlier_probability((c1, c2, r), d2)
        assert np.all(np.isfinite(fast)) and np.all(np.isfinite(exact))
        worst_fast = max(worst_fast, float(np.max(np.abs(fast.astype(np.float64) - want))))
        worst_exact += int(np.count_nonzero(exact != want))
        n_total += d2.size
    note("inlier_probability_fast_max_abs_dev", worst_fast)
    note("inlier_probability_exact_mismatches", f"{worst_exact} of {n_total}")
    assert worst_fast <= bound, worst_fast
    assert worst_exact == 0, f"{worst_exact} of {n_total} values differ from the reference build"


def test_inlier_weight_pair_against_the_reference_build():
    """The deformable sweeps' weight min(pA, pB) in its one-exponential form (k_links.hip.h inlier_weight_pair) against the
    reference build's getInlierProbability for both images: inside the pair's range and in the general form the VALUE is
    within INLIER_PROBABILITY_BOUND = 2^-16; a weight the sweep drops without asking for its range (form 2: below
    threshold - 1e-4 in the one-exponential form) is below the threshold in the reference build too.  Mixtures: the
    benchmark's (c1 3, c2 200), wide outlier components (the eps of stats.h:91 matters most there), a mixture with
    c1 > c2 and degenerate ratios (no range: general form), and two thresholds."""
    if ref_lib() is None:
        pytest.fail("oracle/_ref/libfrog_refstats.so (the reference's stats.cxx) was not built")
    bound = 2.0 ** -16
    mixtures = [(3.0, 200.0, 0.7), (3.3, 205.0, 0.69), (0.8, 60.0, 0.5), (10.0, 300.0, 0.05), (2.0, 1000.0, 0.95),
                (40.0, 300.0, 0.5), (5.0, 3.0, 0.5), (3.0, 200.0, 1e-6), (3.0, 200.0, 1.0 - 1e-6), (1e-3, 50.0, 0.5)]
    rng = np.random.default_rng(7)
    worst, worst_at, n_form = 0.0, None, np.zeros(3, np.int64)
    for threshold in (0.5, 0.1):
        for ia, ma in enumerate(mixtures):
            for mb in mixtures[ia::3]:
                ra, rb = Stats("ref"), Stats("ref")
                ra.set_params(list(ma)); rb.set_params(list(mb))
                cs = min(ma[0], mb[0])
                d = np.concatenate([
                    cs * np.geomspace(0.02, 60.0, 30000),
                    np.linspace(0.0, 0.2, 1001),
                    np.nextafter(np.float32(0.1), np.float32([0.0, 1.0])),
                    rng.uniform(0.0, 5.0 * max(ma[1], mb[1]), 20000),
                ]).astype(np.float32)
                d2 = (d * d).astype(np.float32)
                d2 = np.concatenate([d2, np.nextafter(np.float32(0.01), np.float32([0.0, 1.0])), np.float32([0.01])])
                root = np.sqrt(d2)
                want = np.minimum(ra.prob_n(root), rb.prob_n(root)).astype(np.float64)
                # a dense stretch where the pair's weight crosses the threshold
                k = int(np.argmin(np.abs(want[:30000] - threshold)))
                dense = (d[k] + np.arange(-5000, 5000) * np.spacing(d[k])).astype(np.float32)
                d2 = np.concatenate([d2, (dense * dense).astype(np.float32)])
                root = np.sqrt(d2)
                want = np.minimum(ra.prob_n(root), rb.prob_n(root)).astype(np.float64)
                w, form = device_inlier_weight_pair(ma, mb, d2, threshold)
                value = form < 2
                assert np.all(np.isfinite(w[value]))
                dev = np.abs(w[value].astype(np.float64) - want[value])
                if dev.size and dev.max() > worst:
                    worst, worst_at = float(dev.max()), (ma, mb, threshold, float(d2[value][int(np.argmax(dev))]), int(form[value][int(np.argmax(dev))]))
                # dropped without a range: an outlier in the reference build as well, by a margin
                assert np.all(want[form == 2] < threshold - 5e-5), (ma, mb, threshold)
                assert np.all(w[form == 2] < threshold - 1e-4 + 1e-9)
                n_form += np.bincount(form, minlength=3)[:3]
    note("inlier_weight_pair_max_abs_dev", f"{worst} at {worst_at}")
    note("inlier_weight_pair_forms_one_exp_general_dropped", n_form.tolist())
    assert worst <= bound, (worst, worst_at)
    assert n_form[0] > 0 and n_form[1] > 0 and n_form[2] > 0


def test_inlier_weight_pair_random_mixtures():
    """scripts/fuzz_weight_pair.py in small: 60 random pairs of mixtures (c1 over four decades, c2 / c1 from 0.5 to 1000, ratios
    down to 1e-6 and up to 1 - 1e-6) and thresholds from 0.01 to 0.99 -- VALUES within 2^-16 of the reference build, no link that
    the reference build calls an inlier dropped.  (400 pairs, same generator: worst 7.1e-6.)"""
    if ref_lib() is None:
        pytest.fail("oracle/_ref/libfrog_refstats.so (the reference's stats.cxx) was not built")
    rng = np.random.default_rng(123)
    worst = 0.0
    for _ in range(60):
        def mix():
            c1 = float(np.float32(10.0 ** rng.uniform(-2, 2)))
            c2 = float(np.float32(c1 * 10.0 ** rng.uniform(-0.3, 3)))
            r = float(np.float32(rng.choice([rng.uniform(0.01, 0.99), 10.0 ** rng.uniform(-6, -2), 1 - 10.0 ** rng.uniform(-6, -2)])))
            return (c1, c2, r)
        ma, mb = mix(), mix()
        thr = float(rng.choice([0.5, 0.5, 0.1, 0.9, 0.01, 0.99]))
        ra, rb = Stats("ref"), Stats("ref")
        ra.set_params(list(ma)); rb.set_params(list(mb))
        d = np.concatenate([min(ma[0], mb[0]) * np.geomspace(0.01, 80.0, 20000), rng.uniform(0, 5 * max(ma[1], mb[1]), 5000),
                            np.linspace(0, 0.3, 301)]).astype(np.float32)
        d2 = (d * d).astype(np.float32)
        want = np.minimum(ra.prob_n(np.sqrt(d2)), rb.prob_n(np.sqrt(d2))).astype(np.float64)
        k = int(np.argmin(np.abs(want - thr)))
        dense = (d[k] + np.arange(-2000, 2000) * np.spacing(d[k])).astype(np.float32)
        d2 = np.concatenate([d2, (dense * dense).astype(np.float32)])
        want = np.minimum(ra.prob_n(np.sqrt(d2)), rb.prob_n(np.sqrt(d2))).astype(np.float64)
        w, form = device_inlier_weight_pair(ma, mb, d2, thr)
        value = form < 2
        assert np.all(np.isfinite(w[value])), (ma, mb, thr)
        if value.any():
            worst = max(worst, float(np.max(np.abs(w[value].astype(np.float64) - want[value]))))
        assert not np.any(want[form == 2] >= thr), (ma, mb, thr)
    note("inlier_weight_pair_random_mixtures_max_abs_dev", worst)
    assert worst <= 2.0 ** -16, worst


# ---- integer outputs, exactly -------------------------------------------------------------------------------

def lockstep_to_deformable(pairs, iters=20, **opt):
    """Both sides free-running through the linear stage, then re-based; returns (g, ref)."""
    g = ImageGroup(pairs, **opt)
    ref = OracleGroup(pairs.model, _abi.FrogOptions.default(**opt))
    ref.setup_stats()
    schedule.run([g, ref], iters, [])
    return g, ref


def same_inputs(g, ref):
    """Identical coordinates and mixtures on both sides: what an integer comparison needs."""
    g.set_points2(ref.xyz2())
    for i in range(ref.n_images):
        g.set_em(i, ref.em(i))


def census_equal(g, ref, images=None):
    c = g.countInliers()
    rc = ref.count_inliers((_abi.FrogCounts * ref.n_images)())
    for i in (images if images is not None else range(ref.n_images)):
        assert (c[i].points, c[i].pairs, c[i].inliers, c[i].outliers) == \
               (rc[i].points, rc[i].pairs, rc[i].inliers, rc[i].outliers), f"census of image {i}"
        assert (c[i].c1, c[i].c2, c[i].ratio) == (rc[i].c1, rc[i].c2, rc[i].ratio)
    return c


def test_census_is_exact_on_identical_inputs(small_pairs):
    """countInliers (imageGroup.cxx:988-1060) is integer work: with the same xyz2 and (c1, c2, ratio) on both sides
    every per-image count must be equal -- the weight of a link near the threshold is decided by the reference's own
    arithmetic on the device (k_links.hip.h THRESHOLD_BAND)."""
    for thr in (0.5, 0.3, 0.9):
        g, ref = lockstep_to_deformable(small_pairs, inlier_threshold=thr)
        same_inputs(g, ref)
        census_equal(g, ref)
        # and again in the deformable stage, after a few steps on a lattice
        g.setupDeformableTransforms(1); ref.deformable_setup(1, _abi.FrogGridInfo())
        g.transformPoints(); ref.transform_points()
        for _ in range(3):
            g.updateDeformableTransforms(0.02); ref.deformable_step(0.02)
            g.transformPoints(); ref.transform_points()
        same_inputs(g, ref)
        census_equal(g, ref)


def test_census_exact_with_sub_passes_and_wide_records(small_pairs, monkeypatch):
    monkeypatch.setenv("FROG_SUBPASSES", "2")
    monkeypatch.setenv("FROG_WIDE_RECORDS", "1")
    g, ref = lockstep_to_deformable(small_pairs)
    same_inputs(g, ref)
    census_equal(g, ref)


def test_em_parameters_bit_exact_after_every_refresh(small_pairs):
    """updateStats three times in a row on identical coordinates: ordinals, samples, histogram bins AND the fitted
    (c1, c2, ratio) are equal bit for bit (the EM's f32 sums run in sample order on the device, stats.cxx:28-40)."""
    for max_size in (10000, 2000):
        g = ImageGroup(small_pairs, stats_max_size=max_size)
        ref = OracleGroup(small_pairs.model, _abi.FrogOptions.default(stats_max_size=max_size))
        ref.setup_stats()
        g.setupLinearTransforms(); ref.linear_init()
        g.transformPoints(); ref.transform_points()
        for refresh in range(3):
            g.updateStats(); ref.update_stats()
            for i in range(small_pairs.n_images):
                s, o = g.samples(i)
                rs, ro = ref.samples(i)
                assert np.array_equal(o, ro) and np.array_equal(s, rs)
                assert np.array_equal(g.histogram(i), ref.histogram(i))
                assert np.array_equal(g.em(i), ref.em(i)), f"EM of image {i}, refresh {refresh}: {g.em(i)} vs {ref.em(i)}"


# ---- the parity sweep ---------------------------------------------------------------------------------------

SWEEP = [(dict(n=6, pts=3000, ppb=1500, seed=s), {}) for s in (1, 2, 3)] + [
    (dict(n=6, pts=3000, ppb=1500, seed=4), dict(use_scale=0)),
    (dict(n=6, pts=3000, ppb=1500, seed=5), dict(inlier_threshold=0.3)),
    (dict(n=6, pts=3000, ppb=1500, seed=6), dict(guarantee_diffeomorphism=0)),
    (dict(n=6, pts=3000, ppb=1500, seed=7), dict(initial_grid_size=60.0)),
    (dict(n=6, pts=3000, ppb=1500, seed=8), dict(max_displacement_ratio=0.2)),
    (dict(n=10, pts=1500, ppb=600, seed=9), dict(stats_max_size=3000)),
    (dict(n=3, pts=6000, ppb=4000, seed=10), dict(linear_alpha=0.3)),
]
from lattice_util import compare_lattice, node_weights      # noqa: E402  (the criterion is explained there)


@pytest.mark.parametrize("case", range(len(SWEEP)))
def test_parity_sweep(case):
    """Full schedule (50 linear + 3 levels x 40, regrids included), both sides free-running from the same pairs.
    Asserted for EVERY case, with no case-dependent exemption:
      * lattices per level, energy series (1e-4), matrices (1e-4);
      * coefficients of every control point, weighted by how well the group's points determine its node
        (tests/lattice_util.py): |c - c_ref| w <= 1e-4 max|c_ref|, w = min(1, smallest non-zero support over the images);
      * the displacement field of every lattice evaluated at EVERY point of its image: <= 1e-4 of the largest displacement;
      * the final coordinates.
    and every coefficient, unweighted, within 3e-3 (lattice_util.RIM_REL)."""
    cfg, opt = SWEEP[case]
    pairs = Pairs.synthetic(cfg["n"], cfg["pts"], cfg["ppb"], seed=cfg["seed"])
    g = ImageGroup(pairs, **opt)
    ref = OracleGroup(pairs.model, _abi.FrogOptions.default(**opt))
    ref.setup_stats()
    po = np.asarray(pairs.point_offset)
    snapshots = []                      # per lattice: the reference's re-based coordinates it acts on
    worst = {"E": 0.0}

    def on(tag, sides, e=None, infos=None):
        kind = schedule.kind(tag)
        if kind == "setup":
            snapshots.append(ref.xyz().copy())
        elif kind in ("linear", "deformable"):
            worst["E"] = max(worst["E"], abs(e[0] - e[1]) / e[1])
    # (the driver asserts at every step that both sides' guards decide alike)
    schedule.run([g, ref], 50, [40] * 3, on=on)
    worst_e = worst["E"]
    assert g.num_grids() == ref.num_grids() == len(snapshots)
    assert worst_e < REL
    for i in range(pairs.n_images):
        m, mr = g.matrix(i), ref.matrix(i)
        assert relerr(np.diag(m)[:3], np.diag(mr)[:3]) < REL and relerr(m[:3, 3], mr[:3, 3]) < REL
    worst_c, worst_d, n_unsupported, n_cp_total = 0.0, 0.0, 0, 0
    for k in range(ref.num_grids()):
        w = node_weights(ref, k, po, snapshots[k])
        for i in range(pairs.n_images):
            dev_c, dev_d, n_ex, n_cp = compare_lattice(g, ref, k, i, snapshots[k][po[i]:po[i + 1]], w)
            n_unsupported += n_ex; n_cp_total += n_cp
            worst_c, worst_d = max(worst_c, dev_c), max(worst_d, dev_d)
            assert dev_c <= REL, f"lattice {k} image {i}: supported coefficients off by {dev_c:.2e}"
            assert dev_d <= REL, f"lattice {k} image {i}: displacement field off by {dev_d:.2e}"
    assert relerr(g.points()[0], ref.xyz()) < 1e-6
    note(f"parity_sweep_case_{case}", f"E {worst_e:.2e} coeff {worst_c:.2e} field {worst_d:.2e} "
                                     f"nodes_weighted_below_1 {n_unsupported}/{n_cp_total}")


# ---- certified outlier culling ---------------------------------------------------------------------------------

@pytest.mark.parametrize("opt", [{}, dict(inlier_threshold=0.2), dict(guarantee_diffeomorphism=0)])
def test_culled_sweep_is_bit_identical_to_the_full_sweep(small_pairs, monkeypatch, opt):
    """k_cull.hip.h: the deformable sweep walks only the half-links that are not provably outliers.  Whole runs with
    the list (default skin), with a zero skin (the list is out of date after every step: full sweep + rebuild each
    iteration) and without culling give the same bits everywhere."""
    g0, E0, L0, S0, C0, X0 = _run_schedule(small_pairs, monkeypatch, False, **opt)
    g1, E1, L1, S1, C1, X1 = _run_schedule(small_pairs, monkeypatch, True, **opt)
    g2, E2, L2, S2, C2, X2 = _run_schedule(small_pairs, monkeypatch, True, skin="1.0,0.0", **opt)
    assert g0.gridsPerLevel == g1.gridsPerLevel == g2.gridsPerLevel
    assert E0 == E1 == E2
    for a, b, c in zip(L0, L1, L2):
        for x, y, z in zip(a, b, c):
            assert np.array_equal(x, y) and np.array_equal(x, z)
    assert np.array_equal(S0, S1) and np.array_equal(S0, S2) and C0 == C1 == C2
    assert np.array_equal(X0, X1) and np.array_equal(X0, X2)
    built0, listed0, owned0 = g0.cull_stats()
    built1, listed1, owned1 = g1.cull_stats()
    built2, listed2, owned2 = g2.cull_stats()
    assert built0 == 0 and listed0 == 0
    assert 1 <= built1 <= 10 and 0 < listed1 < owned1 == small_pairs.n_half_links     # the false matches are left out
    assert built2 > 20                                                               # zero skin: rebuilt all the time
    ranges, elected = g1.cull_ranges()
    assert 0 <= elected < ranges          # 128 links per tile and partner image: most steps cannot hold a point twice
    note("cull_small_pairs", f"builds {built1} listed {listed1} of {owned1}; zero skin builds {built2}; "
                             f"ranges {ranges}, with election {elected}")


def test_culled_sweep_with_and_without_lane_election(monkeypatch):
    """The list builder certifies, per (tile, partner group) range, that no step of 64 listed records holds a point
    twice; such ranges are swept without the lane election (k_cull.hip.h CULL_DUP_BIT).  A group of many small images
    has ranges of both kinds (a step spans several partner images): same bits as the full sweep, which always elects."""
    pairs = Pairs.synthetic(24, 400, 150, seed=5)
    g0, E0, L0, S0, C0, X0 = _run_schedule(pairs, monkeypatch, False)
    g1, E1, L1, S1, C1, X1 = _run_schedule(pairs, monkeypatch, True)
    assert g0.gridsPerLevel == g1.gridsPerLevel and E0 == E1
    for a, b in zip(L0, L1):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    assert np.array_equal(S0, S1) and C0 == C1 and np.array_equal(X0, X1)
    ranges, elected = g1.cull_ranges()
    assert 0 < elected < ranges
    note("cull_many_small_images", f"ranges {ranges}, with election {elected}")


def test_list_written_by_the_sweep_equals_the_list_of_the_build_pass(small_pairs, monkeypatch):
    """The sweep that walks every record writes the next culling list as it goes (k_links.hip.h BUILD); the stand-alone
    pass (cull_build_kernel, FROG_CULL_BUILD_PASS=1: what wide records still use) must list the same half-links and flag
    the same ranges, and the runs must agree bit for bit."""
    monkeypatch.delenv("FROG_CULL_BUILD_PASS", raising=False)
    g1, E1, L1, S1, C1, X1 = _run_schedule(small_pairs, monkeypatch, True, skin="1.2,3.0")
    monkeypatch.setenv("FROG_CULL_BUILD_PASS", "1")
    g2, E2, L2, S2, C2, X2 = _run_schedule(small_pairs, monkeypatch, True, skin="1.2,3.0")
    assert E1 == E2 and C1 == C2 and np.array_equal(S1, S2) and np.array_equal(X1, X2)
    for a, b in zip(L1, L2):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    assert g1.cull_stats() == g2.cull_stats() and g1.cull_stats()[0] >= 2        # a thin skin: several lists per run
    assert g1.cull_ranges() == g2.cull_ranges()


def test_culling_follows_coordinates_and_mixtures_set_from_outside(small_pairs):
    """The check before every sweep looks at the coordinates and mixtures as they ARE: overwriting xyz2 or the EM
    parameters between two steps (test hooks) must not leave a stale list in use."""
    g, ref = lockstep_to_deformable(small_pairs)
    g.setupDeformableTransforms(1); ref.deformable_setup(1, _abi.FrogGridInfo())
    g.transformPoints(); ref.transform_points()
    g.updateStats(); ref.update_stats()
    same_inputs(g, ref)
    e, er = g.updateDeformableTransforms(0.0), ref.deformable_step(0.0)            # alpha 0: builds the list, moves nothing
    assert abs(e - er) / er < 1e-6
    assert relerr(g.point_sums(), ref.point_sums()) < 1e-5
    # (a) a wide mixture for image 0: its certified cutoff grows past the list's -> the next sweep must see the
    #     links that were left out; the oracle is the witness
    wide = np.array([60.0, 300.0, 0.9], np.float32)
    g.set_em(0, wide); ref.set_em(0, wide)
    e, er = g.updateDeformableTransforms(0.0), ref.deformable_step(0.0)
    assert abs(e - er) / er < 1e-6 and relerr(g.point_sums(), ref.point_sums()) < 1e-5
    # (b) image 1 moved by 150 mm: links that were far are now near
    x = ref.xyz2().copy()
    po = np.asarray(small_pairs.point_offset)
    x[po[1]:po[2]] += np.float32(150.0)
    g.set_points2(x); ref.set_xyz2(x)
    e, er = g.updateDeformableTransforms(0.0), ref.deformable_step(0.0)
    assert abs(e - er) / er < 1e-6 and relerr(g.point_sums(), ref.point_sums()) < 1e-5
    assert g.cull_stats()[0] >= 2          # the host was told to rebuild


# ---- layout edge cases --------------------------------------------------------------------------------------

def many_tiny_images(n_images, pts, seed=3):
    rng = np.random.default_rng(seed)
    cloud = rng.uniform(0, 200, size=(pts, 3))
    po = np.arange(n_images + 1) * pts
    xyz = np.concatenate([(cloud + rng.normal(0, 1.0, (pts, 3)) + rng.uniform(-5, 5, 3)).astype(np.float32)
                          for _ in range(n_images)])
    blocks = []
    for i in range(n_images):
        for j in (i + 1, i + 7, i + 1200):
            if j < n_images:
                p = np.arange(pts, dtype=np.uint32)
                blocks.append((i, j, p, p[::-1].copy() if (i + j) % 5 == 0 else p))
    return Pairs.from_arrays(po, xyz, blocks)


def test_more_than_2048_images(monkeypatch):
    """3000 images of 4 points: partner groups of 375 images (9 bits).  The 4-byte record form keeps a group's constants
    in 256-entry LDS tables, so this model must take the 8-byte form (prep.h) -- and agree with the oracle."""
    pairs = many_tiny_images(3000, 4)
    g = ImageGroup(pairs)
    ref = OracleGroup(pairs.model, _abi.FrogOptions.default())
    ref.setup_stats()
    g.setupLinearTransforms(); ref.linear_init()
    g.transformPoints(); ref.transform_points()
    assert np.array_equal(g.points()[1], ref.xyz2())
    g.updateStats(); ref.update_stats()
    for i in (0, 1, 1500, 2999):
        assert np.array_equal(g.samples(i)[0], ref.samples(i)[0]) and np.array_equal(g.em(i), ref.em(i))
    for _ in range(3):
        e, er = g.updateLinearTransforms(), ref.linear_step()
        g.transformPoints(); ref.transform_points()
        assert abs(e - er) / er < 1e-5
    same_inputs(g, ref)
    census_equal(g, ref, images=range(0, 3000, 37))
    g.transformPoints(True); ref.transform_points(True)
    g.setupDeformableTransforms(0); ref.deformable_setup(0, _abi.FrogGridInfo())
    g.transformPoints(); ref.transform_points()
    same_inputs(g, ref)
    e, er = g.updateDeformableTransforms(0.02), ref.deformable_step(0.02)
    assert (e < 0) == (er < 0)
    assert relerr(g.point_sums(), ref.point_sums()) < 1e-5


def test_blocks_in_shuffled_file_order():
    """pairs.bin from another producer: blocks in arbitrary order, some (j, i) with j > i.  The device sums a point's
    links partner-image ascending inside each partner group, the reference in file order (prep.h header): last-ulp
    differences in the f32 per-point sums, nothing more."""
    rng = np.random.default_rng(11)
    src = Pairs.synthetic(6, 2000, 900, seed=12)
    po = np.asarray(src.point_offset)
    blocks = []
    for b in range(src.n_blocks):
        i1, i2, p1, p2 = src.block(b)
        if rng.random() < 0.5:
            order = np.argsort(p2, kind="stable")
            blocks.append((i2, i1, p2[order].copy(), p1[order].copy()))     # written from the other image's side
        else:
            blocks.append((i1, i2, p1.copy(), p2.copy()))
    blocks = [blocks[k] for k in rng.permutation(len(blocks))]
    pairs = Pairs.from_arrays(po, np.asarray(src.xyz), blocks)
    assert pairs.n_pairs == src.n_pairs
    g, ref = lockstep_to_deformable(pairs, iters=12)
    g.setupDeformableTransforms(1); ref.deformable_setup(1, _abi.FrogGridInfo())
    g.transformPoints(); ref.transform_points()
    g.updateStats(); ref.update_stats()
    for i in range(pairs.n_images):
        assert np.array_equal(g.samples(i)[1], ref.samples(i)[1])          # ordinals follow the file's link order
    same_inputs(g, ref)
    snapshot = ref.xyz().copy()
    e, er = g.updateDeformableTransforms(0.02), ref.deformable_step(0.02)
    assert er > 0 and abs(e - er) / er < 1e-6
    assert relerr(g.point_sums(), ref.point_sums()) < 1e-5
    w = node_weights(ref, 0, po, snapshot)
    for i in range(pairs.n_images):
        # same criterion as the parity sweep: the summation order differs from the file's here, and a control point on
        # the rim of the box turns one ulp of a per-point sum into 1e-4 of its value
        dev_c, dev_d, _, _ = compare_lattice(g, ref, 0, i, snapshot[po[i]:po[i + 1]], w)
        assert dev_c <= REL and dev_d <= REL, (i, dev_c, dev_d)
    same_inputs(g, ref)
    census_equal(g, ref)


def test_duplicate_links_are_added_in_the_reference_order():
    """Every linked pair closer than 0.1 mm has weight exactly 1 on both sides (stats.h:87), so the f32 per-point sums
    (imageGroup.cxx:270-278) depend on the ORDER of the adds and on nothing else: three links of every point of image 0
    into image 1, in steps where all 64 lanes carry duplicates and the points k and k + 128 of a tile share an election
    word (k_links.hip.h).  Bit-equal sums = the reference's order."""
    rng = np.random.default_rng(21)
    n = 700
    a = rng.uniform(0, 200, (n, 3)).astype(np.float32)
    b = (np.repeat(a, 3, axis=0) + rng.uniform(-0.025, 0.025, (3 * n, 3))).astype(np.float32)
    pairs = Pairs.from_arrays([0, n, 4 * n], np.concatenate([a, b]),
                              [(0, 1, np.repeat(np.arange(n), 3).astype(np.uint32), np.arange(3 * n, dtype=np.uint32))])
    g = ImageGroup(pairs)
    ref = OracleGroup(pairs.model, _abi.FrogOptions.default())
    ref.setup_stats()
    g.setupLinearTransforms(); ref.linear_init()
    g.transformPoints(); ref.transform_points()
    g.transformPoints(True); ref.transform_points(True)
    g.setupDeformableTransforms(0); ref.deformable_setup(0, _abi.FrogGridInfo())
    g.transformPoints(); ref.transform_points()
    g.updateStats(); ref.update_stats()
    same_inputs(g, ref)
    x2 = ref.xyz2()
    d = np.linalg.norm(np.repeat(x2[:n], 3, axis=0) - x2[n:], axis=1)
    assert d.max() < 0.095                                  # every weight is the constant 1
    e, er = g.updateDeformableTransforms(0.02), ref.deformable_step(0.02)
    ps, rps = np.asarray(g.point_sums()), np.asarray(ref.point_sums())
    assert np.all(rps[:n, 3] == 3.0) and np.all(rps[n:, 3] == 1.0)
    assert np.array_equal(ps, rps)
    assert abs(e - er) <= 1e-6 * abs(er)


@pytest.mark.parametrize("energy_pass", [False, True])
def test_points_outside_the_lattice_take_the_stray_path(small_pairs, monkeypatch, energy_pass):
    """A lattice whose box does not hold every point (a host that hands frog_deformable_setup_bounds a box of its own:
    the reference would write outside its gradient array, imageGroup.cxx:303-331).  Here such points are clamped into a
    rim brick, their taps inside the lattice go to the gradient lattice with atomics and the lattice step folds them in
    (k_grid.hip.h "stray").  The per-step counter is double-buffered by step parity since the energy reduction moved
    onto the scatter's launch: several steps in a row must each see their own count."""
    from frog_amd.distributed import HipEngine
    if energy_pass:
        monkeypatch.setenv("FROG_ENERGY_PASS", "1")         # the energy reduction as a launch of its own: the other way the counters are reset
    else:
        monkeypatch.delenv("FROG_ENERGY_PASS", raising=False)
    n = small_pairs.n_images
    eng = HipEngine(small_pairs, _abi.FrogOptions.default(), 0, (0, n))
    eng.linear_init((0.5, 0.5, 0.5)); eng.transform_points_local(False)
    eng.update_stats_local(); eng.stats_publish()
    for _ in range(4):
        eng.linear_step_local(); eng.energy_read(); eng.transform_points_local(False)
    eng.transform_points_local(True)
    mn, mx = eng.bounds_local()
    c, h = 0.5 * (mn[0] + mx[0]), 0.30 * (mx[0] - mn[0])            # 60 % of the cloud's extent in x (+ the 20 % margin)
    eng.deformable_setup_bounds(1, [c - h, mn[1], mn[2]], [c + h, mx[1], mx[2]])
    eng.transform_points_local(False)
    eng.update_stats_local(); eng.stats_publish()
    lib = _abi.hip_lib()
    counts, E = [], []
    for it in range(5):
        eng.phase_a(0.02); eng.phase_b()
        E.append(eng.phase_c())
        eng.transform_points_local(False)
        k = C.c_uint64()
        assert lib.frog_test_stray_points(eng._ctx, C.byref(k)) == 0
        counts.append(k.value)
    per_step = np.diff([0] + counts)
    assert per_step[0] > 0 and np.all(per_step == per_step[0])        # the same points every step (they do not move in xyz)
    assert all(np.isfinite(E)) and all(e > 0 for e in E)
    for i in range(n):
        cf = eng.grid(i, eng.num_grids() - 1)[1]
        assert np.all(np.isfinite(cf)) and np.abs(cf).max() > 0
    x, x2 = eng.points()
    assert np.all(np.isfinite(x2))
    eng.close()
    # both ways of reducing the energy see the same steps (float atomics of the stray taps: not the same bits)
    seen = test_points_outside_the_lattice_take_the_stray_path.__dict__.setdefault("seen", {})
    seen[energy_pass] = (per_step[0], E)
    if len(seen) == 2:
        assert seen[False][0] == seen[True][0]
        assert np.allclose(seen[False][1], seen[True][1], rtol=1e-5)


def test_brick_edge_8_equals_brick_edge_4(small_pairs, monkeypatch):
    """Sparse lattices (fewer than 24 points per 4^3-cell brick) use bricks of 8^3 cells in the scatter: 11^3-node tiles,
    another sort key.  Forced on a small group (FROG_BRICK): same lattices as with edge 4 up to the order of the f32
    additions, no point outside the brick it was sorted into."""
    def run(brick):
        monkeypatch.setenv("FROG_BRICK", str(brick))
        g = ImageGroup(small_pairs)
        g.linearIterations, g.deformableLevels, g.deformableIterations = 12, 3, 10
        E = g.run()
        assert g.stray_points() == 0
        return E, [[g.grid(i, k)[1] for k in range(g.num_grids())] for i in range(small_pairs.n_images)], g.gridsPerLevel
    E4, L4, G4 = run(4)
    E8, L8, G8 = run(8)
    assert G4 == G8 and len(E4) == len(E8)
    assert np.max(np.abs(np.array(E4) - np.array(E8)) / np.array(E4)) < 1e-6
    for a, b in zip(L4, L8):
        for x, y in zip(a, b):
            assert np.max(np.abs(x - y)) <= 1e-3 * max(float(np.max(np.abs(x))), 1e-30)      # rim nodes: tests/lattice_util.py
    assert relerr(np.concatenate([l[-1] for l in L8]), np.concatenate([l[-1] for l in L4])) < 1e-3


def test_tiled_transform_equals_pointwise(small_pairs, monkeypatch):
    """transformPoints through a lattice (vtkBSplineTransform): the form that keeps a brick's coefficients in LDS as f64
    (one wavefront per scatter block) against the thread-per-point form (FROG_K11_POINTWISE=1) -- the same operations in
    the same order on the same values: every coordinate of a whole run has the same bits."""
    def run(pointwise):
        if pointwise:
            monkeypatch.setenv("FROG_K11_POINTWISE", "1"); monkeypatch.delenv("FROG_K11_TILED", raising=False)
        else:
            monkeypatch.delenv("FROG_K11_POINTWISE", raising=False); monkeypatch.setenv("FROG_K11_TILED", "1")
        g = ImageGroup(small_pairs)
        g.linearIterations, g.deformableLevels, g.deformableIterations = 10, 3, 12
        E = g.run()
        return E, g.points(), [g.grid(i, g.num_grids() - 1)[1] for i in range(small_pairs.n_images)]
    E0, (x0, y0), L0 = run(True)
    E1, (x1, y1), L1 = run(False)
    assert E0 == E1 and np.array_equal(x0, x1) and np.array_equal(y0, y1)
    for a, b in zip(L0, L1):
        assert np.array_equal(a, b)


def test_context_that_owns_only_empty_images():
    """A shard may hold only images without points (plan_shards balances half-links): its sweeps have nothing to
    launch, and the split-phase entry points must still succeed with zero sums (no zero-block launch)."""
    rng = np.random.default_rng(2)
    sizes = [300, 0, 0, 250]
    po = np.concatenate([[0], np.cumsum(sizes)])
    xyz = rng.uniform(0, 100, (po[-1], 3)).astype(np.float32)
    p = np.arange(200, dtype=np.uint32)
    pairs = Pairs.from_arrays(po, xyz, [(0, 3, p, p)])
    lib = _abi.hip_lib()
    part = ImageGroup(pairs, image_range=(1, 3))
    part.setupLinearTransforms()
    assert lib.frog_transform_points_local(part._ctx, 0) == _abi.FROG_OK
    assert lib.frog_update_stats_local(part._ctx) == _abi.FROG_OK
    assert lib.frog_stats_publish(part._ctx) == _abi.FROG_OK
    assert lib.frog_linear_step_local(part._ctx) == _abi.FROG_OK, lib.frog_last_error()
    e, nb = C.c_double(), C.c_double()
    assert lib.frog_energy_read(part._ctx, C.byref(e), C.byref(nb)) == _abi.FROG_OK
    c = part.countInliers()
    assert c[1].pairs == 0 and c[2].pairs == 0
    mn, mx = (C.c_double * 3)(), (C.c_double * 3)()
    assert lib.frog_bounds_local(part._ctx, mn, mx) == _abi.FROG_OK
    info = _abi.FrogGridInfo()
    assert lib.frog_deformable_setup_bounds(part._ctx, 0, (C.c_double * 3)(0, 0, 0), (C.c_double * 3)(100, 100, 100),
                                            C.byref(info)) == _abi.FROG_OK, lib.frog_last_error()
    assert lib.frog_deformable_phase_a(part._ctx, 0.02) == _abi.FROG_OK, lib.frog_last_error()
    assert lib.frog_deformable_phase_b(part._ctx) == _abi.FROG_OK
    assert lib.frog_deformable_phase_c(part._ctx, C.byref(e)) == _abi.FROG_OK
