"""The culling list's certificate (frog_amd/csrc/device/k_cull.hip.h), part by part, on mixtures, geometry and motion
designed for it: (a) what a per-image cutoff claims, against the device's own weight and the reference build; (b) which
half-links a list holds, at the floats around the rule's edge; (c) the staleness check, at the floats around the allowance;
(d) whole schedules with skins of a millimetre, through every kernel that measures the displacement.  The restatement is
tests/cull_restate.py; the read-back is frog_test_cull_readback."""
import ctypes as C
import functools

import numpy as np
import pytest

import cull_restate as cr
from frog_amd import _abi, schedule
from frog_amd.image_group import ImageGroup, device_inlier_probability
from frog_amd.pairs import Pairs
from oracle.oracle_api import Stats, ref_lib
from gpu_util import note
from test_gpu_round2 import MIXTURES, many_tiny_images

pytestmark = pytest.mark.gpu
F = np.float32
INF = F(np.inf)
THRESHOLD_BAND = F(1e-4)            # k_links.hip.h


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def need_ref():
    if ref_lib() is None:
        pytest.fail("oracle/_ref/libfrog_refstats.so (the reference's stats.cxx) was not built")


# ---- (a) the cutoffs certify what they claim -------------------------------------------------------------------------------

def _tables():
    """Rows of (c1, c2, ratio) in tables of 64: the mixtures of test_gpu_round2.py, its random generator, c1 close to c2,
    ratios at both ends, and the rows that must have no cutoff."""
    rows = [tuple(m) for m in MIXTURES]
    rng = np.random.default_rng(123)
    for _ in range(120):                                    # test_inlier_weight_pair_random_mixtures' generator
        c1 = float(F(10.0 ** rng.uniform(-2, 2)))
        c2 = float(F(c1 * 10.0 ** rng.uniform(-0.3, 3)))
        r = float(F(rng.choice([rng.uniform(0.01, 0.99), 10.0 ** rng.uniform(-6, -2), 1 - 10.0 ** rng.uniform(-6, -2)])))
        rows.append((c1, c2, r))
    for c1 in (0.05, 0.8, 3.0, 40.0):
        for q in (1.0 + 2.0 ** -20, 1.001, 1.1):
            rows.append((c1, float(F(F(c1) * F(q))), 0.5))
        for r in (1e-6, 1.0 - 1e-6):
            rows += [(c1, 60.0 * c1, r), (c1, float(F(F(c1) * F(1.1))), r)]
    rows += [(5.0, 3.0, 0.5), (3.0, 3.0, 0.5), (3.0, 200.0, 0.0), (3.0, 200.0, 1.0), (3.0, 200.0, -0.1), (3.0, 200.0, 1.5),
             (3.0, 200.0, np.nan), (0.0, 200.0, 0.5), (3.0, np.inf, 0.5), (3.0, 1e30, 0.5)]
    rows = [tuple(float(F(v)) for v in r) for r in rows]
    while len(rows) % 64:
        rows.append(rows[len(rows) % len(MIXTURES)])
    return [rows[k:k + 64] for k in range(0, len(rows), 64)]


def _d2_sets(cut):
    """The squared distances behind a cutoff: the 4 096 consecutive floats upward from cut^2 and 20 000 up to (1e3 cut)^2."""
    c2 = F(F(cut) * F(cut))
    dense = (bits(c2).astype(np.uint32) + np.arange(4096, dtype=np.uint32)).view(F)
    with np.errstate(over="ignore"):
        wide = np.geomspace(float(c2), (1e3 * float(cut)) ** 2, 20000).astype(F)
    wide = wide[np.isfinite(wide) & (wide >= c2)]
    return np.concatenate([dense, wide])


def _tiny_group(threshold):
    g = ImageGroup(many_tiny_images(64, 8), inlier_threshold=threshold)
    g.setupLinearTransforms(); g.transformPoints()
    return g


def _to_deformable(g):
    g.transformPoints(True)
    g.setupDeformableTransforms(0); g.transformPoints()


@pytest.mark.parametrize("threshold", [0.5, 0.1, 0.99, 1e-3, 9e-4])
def test_deformable_cutoffs_certify_an_outlier(threshold):
    """cut_now of the deformable stage, read back for 192 mixtures: +inf exactly for a degenerate row and for a threshold
    below 1e-3; otherwise finite, at most 1.01 restated + 0.01, and at every squared distance from cut^2 on -- the next 4 096
    floats, 20 000 more up to (1e3 cut)^2 -- the device's fast and exact weights are below threshold - THRESHOLD_BAND and the
    reference build's below the threshold.  At d2 = +inf no weight is below anything: x^2 exp(-x^2 / 2) is inf * 0 = NaN, in the
    reference build as on the device (asserted), so the certificate speaks of finite distances and the list rule must keep an
    infinite one (cull_restate.listed; on the device: test_list_holds_exactly_the_links_the_rule_names)."""
    need_ref()
    t = F(threshold)
    g = _tiny_group(threshold)
    _to_deformable(g)
    worst_excess, n_finite = -np.inf, 0
    for table in _tables():
        g.set_em_rows(table)
        now = g.cull_readback()["cut_now"]
        for em, cut in zip(table, now):
            if cr.degenerate(em, threshold):
                assert cut == INF, (em, threshold, cut)
                continue
            assert np.isfinite(cut), (em, threshold)                    # not useless: a proper mixture has a cutoff
            restated = cr.cull_cutoff_of(em, threshold)
            assert cut <= 1.01 * float(restated) + 0.01, (em, threshold, cut, restated)
            worst_excess = max(worst_excess, (float(cut) - float(restated)) / float(restated))
            n_finite += 1
            d2 = _d2_sets(cut)
            fast, exact = device_inlier_probability(em, d2)
            assert np.all(fast < t - THRESHOLD_BAND), (em, threshold, cut, float(np.nanmax(fast)))
            assert np.all(exact < t - THRESHOLD_BAND), (em, threshold, cut, float(np.nanmax(exact)))
            ref = Stats("ref")
            ref.set_params(list(em))
            assert np.all(ref.prob_n(np.sqrt(d2)) < t), (em, threshold, cut)
            fast, exact = device_inlier_probability(em, np.array([np.inf], F))
            assert np.isnan(ref.prob_n(np.array([np.inf], F))[0]) and np.isnan(fast[0]) and np.isnan(exact[0])
            assert cr.listed(INF, cut, cut)
    if threshold >= 1e-3:
        assert n_finite >= 150
        note(f"cull_cutoff_worst_relative_excess_over_restated_threshold_{threshold}", f"{worst_excess:.3e} ({n_finite} mixtures)")
    else:
        assert n_finite == 0


def test_linear_cutoffs_certify_a_weight_of_exactly_zero():
    """cut_now of the linear stage (the publish of frog_set_em_rows before any lattice): behind a finite cutoff the sweep's weight
    -- fminf of two values of inlier_probability, the function the hook's fast form evaluates (k_links.hip.h, the branch without the
    one-exponential form) -- is +0.0, bit pattern 0, at every squared distance of the three sets; a finite cutoff is at most
    1.01 restated + 0.01.  The linear stage has no threshold: the same cutoffs under a threshold below 1e-3."""
    g = _tiny_group(0.5)
    h = _tiny_group(9e-4)
    worst_excess, n_finite, n_inf = -np.inf, 0, 0
    for table in _tables():
        g.set_em_rows(table); h.set_em_rows(table)
        now = g.cull_readback()["cut_now"]
        assert np.array_equal(bits(now), bits(h.cull_readback()["cut_now"]))
        for em, cut in zip(table, now):
            restated = cr.cull_cutoff_linear_of(em)
            assert np.isfinite(cut) == np.isfinite(restated), (em, cut, restated)
            if not np.isfinite(cut):
                n_inf += 1
                continue
            assert cut <= 1.01 * float(restated) + 0.01, (em, cut, restated)
            worst_excess = max(worst_excess, (float(cut) - float(restated)) / float(restated))
            n_finite += 1
            fast, _ = device_inlier_probability(em, _d2_sets(cut))
            assert not bits(fast).any(), (em, cut, float(np.nanmax(np.abs(fast))))
            assert cr.listed(INF, cut, cut)                 # d2 = +inf: kq1 (inf * 0) is NaN, not +0; the rule keeps the link
    assert n_finite >= 150 and n_inf >= 3
    note("cull_cutoff_linear_worst_relative_excess_over_restated", f"{worst_excess:.3e} ({n_finite} mixtures)")


# ---- (b), (c): a group whose link distances are placed on the rule's edges -----------------------------------------------------

N_IMG, N_PT = 4, 300
EM4 = [(3.0, 200.0, 0.7), (10.0, 300.0, 0.5), (5.0, 100.0, 0.9), (5.0, 3.0, 0.5)]       # the last: no cutoff
EDGE_PAIRS = [(0, 1, 10), (1, 2, 20), (2, 3, 30)]       # (image A, image B, first of three point indices): d2 = cut^2, below, above
K_NAN, K_INF, K_ZERO, K_MOVE = 40, 41, 50, N_PT - 1


def _edge_pairs():
    """4 images of 300 points, every pair of images linked point k to point k in two blocks (0 .. 149, 150 .. 299); point 5 of
    image 0 has a second link into image 1 (to its point 6)."""
    rng = np.random.default_rng(8)
    cloud = rng.uniform(0, 200, (N_PT, 3))
    xyz = np.concatenate([(cloud + rng.normal(0, 15.0, (N_PT, 3))).astype(F) for _ in range(N_IMG)])
    blocks, links = [], []
    for i in range(N_IMG):
        for j in range(i + 1, N_IMG):
            for lo, hi in ((0, 150), (150, 300)):
                p1, p2 = np.arange(lo, hi, dtype=np.uint32), np.arange(lo, hi, dtype=np.uint32)
                if (i, j, lo) == (0, 1, 150):
                    p1, p2 = np.concatenate([p1, [5]]).astype(np.uint32), np.concatenate([p2, [6]]).astype(np.uint32)
                    order = np.argsort(p1, kind="stable")
                    p1, p2 = p1[order], p2[order]
                blocks.append((i, j, p1, p2))
                links += [(i * N_PT + int(a), j * N_PT + int(b), i, j) for a, b in zip(p1, p2)]
    pairs = Pairs.from_arrays(np.arange(N_IMG + 1) * N_PT, xyz, blocks)
    assert pairs.n_half_links == 2 * len(links)
    return pairs, np.array(links, np.int64)


def _offset_with_d2(target):
    """(dx, dy) in f32 with fl(fl(dx dx) + fl(dy dy)) == target: most of the distance along x, the rest along y."""
    target = F(target)
    dx = F(np.sqrt(float(target)) * 0.9)
    for _ in range(4096):
        r = float(target) - float(F(dx * dx))
        dy = F(np.sqrt(max(r, 0.0)))
        for cand in (dy, np.nextafter(dy, F(0)), np.nextafter(dy, INF)):
            if F(F(dx * dx) + F(cand * cand)) == target:
                return dx, cand
        dx = np.nextafter(dx, INF)
    raise AssertionError(f"no f32 offset with squared length {target}")


def _designed_points(base, cut_list, nan_inf=True):
    """The base coordinates with the designed points put in place: three links per EDGE_PAIRS entry at the rule's edge for
    cut = min(cut_list[A], cut_list[B]), a NaN and an infinite coordinate, a link of length 0, and the point that (c) moves at x = 0."""
    x = np.array(base, F).reshape(N_IMG, N_PT, 3).copy()
    targets = {}
    for a, b, k0 in EDGE_PAIRS:
        cut = min(cut_list[a], cut_list[b])
        c2 = F(cut * cut)
        for k, t in zip(range(k0, k0 + 3), (c2, np.nextafter(c2, F(0)), np.nextafter(c2, INF))):
            dx, dy = _offset_with_d2(t)
            x[a, k] = (0.0, 0.0, 0.0)
            x[b, k] = (dx, dy, 0.0)
            targets[(a, b, k)] = t
    if nan_inf:
        x[0, K_NAN, 0] = np.nan
        x[1, K_INF, 0] = np.inf
    x[3, K_ZERO] = x[2, K_ZERO]
    x[3, K_MOVE] = (0.0, 37.0, -12.5)
    return x.reshape(-1, 3), targets


def _deformable_group(pairs, monkeypatch, cull, skin=None, env=()):
    monkeypatch.setenv("FROG_CULL", "1" if cull else "0")
    for name in ("FROG_CULL_SKIN", "FROG_CULL_BUILD_PASS", "FROG_WIDE_RECORDS"):
        monkeypatch.delenv(name, raising=False)
    if skin:
        monkeypatch.setenv("FROG_CULL_SKIN", skin)
    for name in env:
        monkeypatch.setenv(name, "1")
    g = ImageGroup(pairs)
    g.setupLinearTransforms(); g.transformPoints()
    _to_deformable(g)
    g.set_em_rows(EM4)
    return g


def _phase_a(g, alpha=0.0):
    _abi.check(g._lib.frog_deformable_phase_a(g._ctx, alpha), "frog_deformable_phase_a")


def _finish_step(g):
    e = C.c_double()
    _abi.check(g._lib.frog_deformable_phase_b(g._ctx), "frog_deformable_phase_b")
    _abi.check(g._lib.frog_deformable_phase_c(g._ctx, C.byref(e)), "frog_deformable_phase_c")
    return e.value


def _expected_listed(x2, links, cut_list):
    d2 = cr.link_d2(x2, links[:, 0], links[:, 1])
    return d2, cr.listed(d2, np.asarray(cut_list, F)[links[:, 2]], np.asarray(cut_list, F)[links[:, 3]])


@pytest.mark.parametrize("env", [(), ("FROG_CULL_BUILD_PASS",), ("FROG_WIDE_RECORDS",), ("FROG_CULL_BUILD_PASS", "FROG_WIDE_RECORDS")],
                         ids=lambda e: "+".join(e) or "default")
def test_list_holds_exactly_the_links_the_rule_names(monkeypatch, env):
    """Deformable stage, default skin.  Link distances with f32 d2 equal to cut^2, the float below and the float above, for
    cut = min(cut_list[A], cut_list[B]) with the smaller cutoff on A's side (images 0, 1), on B's side (1, 2) and against an
    image without a cutoff (2, 3); a NaN coordinate, an infinite one, a link of length 0, a point with two links into one image.
    One step at alpha 0: the list holds 2 count(listed(...)) half-links, and per-point sums and energy have the bits of a
    context without a list.  (With FROG_CULL_BUILD_PASS that step sweeps the list; otherwise it writes the list while it walks
    every record, and the sweeps of a list are those of test_staleness_at_the_allowance.)"""
    pairs, links = _edge_pairs()
    g = _deformable_group(pairs, monkeypatch, True, env=env)
    now = g.cull_readback()["cut_now"]
    assert now[0] < now[2] < now[1] and now[3] == INF
    cut_list = cr.list_cutoff(now, 2.0, 25.0)
    x2, targets = _designed_points(g.points()[1], cut_list)
    d2, keep = _expected_listed(x2, links, cut_list)
    for (a, b, k), t in targets.items():                    # the designed links have the designed distances
        row = np.nonzero((links[:, 0] == a * N_PT + k) & (links[:, 1] == b * N_PT + k))[0]
        assert len(row) == 1 and d2[row[0]] == t
    edge = [bool(keep[np.nonzero((links[:, 0] == a * N_PT + k) & (links[:, 1] == b * N_PT + k))[0][0]]) for (a, b, k) in targets]
    assert edge == [False, True, False] * 3                 # at cut^2: left out; below: listed; above: left out
    assert 0 < keep.sum() < len(keep) and np.isnan(d2).sum() == 3 and np.isinf(d2).sum() == 3
    g.set_points2(x2)
    e1 = g.updateDeformableTransforms(0.0)
    rb = g.cull_readback()
    assert np.array_equal(bits(rb["cut_list"]), bits(cut_list))
    built, listed, owned = g.cull_stats()
    assert (built, listed, owned) == (1, 2 * int(keep.sum()), pairs.n_half_links)
    s1 = g.point_sums()
    full = _deformable_group(pairs, monkeypatch, False, env=env)
    full.set_points2(x2)
    e0 = full.updateDeformableTransforms(0.0)
    assert np.array_equal(bits(s1), bits(full.point_sums()))
    assert np.float64(e1).view(np.uint64) == np.float64(e0).view(np.uint64), (e1, e0)


def _linear_group(pairs, monkeypatch, cull, env=()):
    monkeypatch.setenv("FROG_CULL", "1")
    monkeypatch.setenv("FROG_CULL_LINEAR", "1" if cull else "0")
    for name in ("FROG_CULL_SKIN_LINEAR", "FROG_CULL_BUILD_PASS", "FROG_WIDE_RECORDS"):
        monkeypatch.delenv(name, raising=False)
    for name in env:
        monkeypatch.setenv(name, "1")
    g = ImageGroup(pairs)
    g.setupLinearTransforms(); g.transformPoints()
    g.set_em_rows(EM4)
    return g


@pytest.mark.parametrize("env", [(), ("FROG_CULL_BUILD_PASS",), ("FROG_WIDE_RECORDS",)], ids=lambda e: "+".join(e) or "default")
def test_linear_list_holds_exactly_the_links_the_rule_names(monkeypatch, env):
    """The same for the linear stage's list (default skin 1.25, 10 mm; frog_cull_stats_linear) against FROG_CULL_LINEAR=0.  With the
    NaN and the infinite coordinate every sum of every image is NaN in both runs, so the count is asserted with them and the values
    without: energies 1e-13, matrices 1e-12, coordinates one f32 ulp, as tests/test_gpu_round3.py compares the two sweeps."""
    pairs, links = _edge_pairs()
    for nan_inf in (True, False):
        g = _linear_group(pairs, monkeypatch, True, env=env)
        now = g.cull_readback()["cut_now"]
        assert np.all(np.isfinite(now)) and now[0] < now[3] and now[2] < now[1]       # (5, 3, 0.5) has an exponent: a cutoff
        cut_list = cr.list_cutoff(now, 1.25, 10.0)
        # the clouds of the four images are closer than these cutoffs: images 1 and 3 are scaled so that some of their links are
        # left out, and not so far that an image is left without a non-zero weight (0 / 0 in its update)
        base = g.points()[1].reshape(N_IMG, N_PT, 3).copy()
        base[1] *= F(1.3); base[3] *= F(0.8)
        x2, targets = _designed_points(base.reshape(-1, 3), cut_list, nan_inf=nan_inf)
        d2, keep = _expected_listed(x2, links, cut_list)
        assert [bool(keep[np.nonzero((links[:, 0] == a * N_PT + k) & (links[:, 1] == b * N_PT + k))[0][0]])
                for (a, b, k) in targets] == [False, True, False] * 3
        assert 0 < keep.sum() < len(keep)
        g.set_points2(x2)
        e1 = g.updateLinearTransforms()
        assert np.array_equal(bits(g.cull_readback()["cut_list"]), bits(cut_list))
        built, listed, owned = g.cull_stats_linear()
        assert (built, listed, owned) == (1, 2 * int(keep.sum()), pairs.n_half_links)
        if nan_inf:
            continue
        full = _linear_group(pairs, monkeypatch, False, env=env)
        full.set_points2(x2)
        e0 = full.updateLinearTransforms()
        g.transformPoints(); full.transformPoints()
        m1, m0 = np.stack([g.matrix(i) for i in range(N_IMG)]), np.stack([full.matrix(i) for i in range(N_IMG)])
        p1, p0 = g.points()[1], full.points()[1]
        assert np.all(np.isfinite(m0)) and np.all(np.isfinite(p0)) and np.isfinite(e0)
        assert abs(e1 - e0) <= 1e-13 * abs(e0)
        assert np.max(np.abs(m1 - m0)) <= 1e-12 * np.max(np.abs(m0))
        assert np.max(np.abs(p1.astype(np.float64) - p0)) <= 1.2e-7 * np.max(np.abs(p0))


# ---- (c) staleness, decision by decision -------------------------------------------------------------------------------------

def _built_thin(pairs, monkeypatch):
    """The group of (b) under the skin 1.0, 1.0, its first list built at the designed coordinates; (group, x2, readback)."""
    g = _deformable_group(pairs, monkeypatch, True, skin="1.0,1.0")
    now = g.cull_readback()["cut_now"]
    cut_list = cr.list_cutoff(now, 1.0, 1.0)
    x2, _ = _designed_points(g.points()[1], cut_list, nan_inf=False)
    g.set_points2(x2)
    _phase_a(g)
    rb = g.cull_readback()
    assert rb["state"] == 0 and rb["disp_n"] == 0 and rb["disp_max"] == 0 and g.cull_stats()[0] == 1
    assert np.array_equal(bits(rb["cut_list"]), bits(cut_list))
    assert bits(rb["allow"]) == bits(cr.allowance(now, cut_list)) and 0.4 < rb["allow"] < 0.5
    _finish_step(g)
    return g, x2, rb


def _moved_step(g, pairs, monkeypatch, x2, moved, rb0):
    """set_points2(moved), one step: disp_max and state as restated; the list is rebuilt by the step after a stale one, and only
    then; per-point sums with the bits of a context without a list."""
    D = cr.disp_of(moved, x2)
    want = cr.stale(rb0["cut_now"], rb0["cut_list"], D)
    listed0 = g.cull_stats()[1]
    g.set_points2(moved)
    _phase_a(g)
    rb = g.cull_readback()
    assert bits(rb["disp_max"]) == bits(D) or (np.isnan(D) and np.isnan(rb["disp_max"])), (rb["disp_max"], D)
    assert rb["state"] == int(want), (D, rb0["allow"])
    _finish_step(g)
    sums = g.point_sums()
    assert g.cull_stats()[:2] == (1, listed0)               # this step swept with the old list, or walked every record
    full = _deformable_group(pairs, monkeypatch, False)
    full.set_points2(moved)
    full.updateDeformableTransforms(0.0)
    assert np.array_equal(bits(sums), bits(full.point_sums()))
    g.set_points2(moved)
    g.updateDeformableTransforms(0.0)
    assert g.cull_stats()[0] == 1 + int(want)               # rebuilt exactly after a stale sweep
    return want


@pytest.mark.parametrize("where", ["below", "at", "above", "edge_below", "edge", "nan"])
def test_staleness_at_the_allowance(monkeypatch, where):
    """Skin 1.0, 1.0.  The last point of the last image (its only, partial, block of CULL_BLOCK_POINTS) moves from x = 0 to
    x = D, so that cull_disp_kernel's f32 distance is D itself: the allowance, the float below it, the float above it, or NaN.
    The read-back shows that D and state = stale(...), and the list is rebuilt exactly after the steps where the state was 1.
    The allowance is a shade (1e-6 relative) below the bound of the stand-alone check, which is the one that runs after
    set_points2: the float above the allowance still passes it.  `edge` is the first float that does not (found on the
    restatement, at most 64 floats up), `edge_below` the one before: the decision flips between them."""
    pairs, _ = _edge_pairs()
    g, x2, rb0 = _built_thin(pairs, monkeypatch)
    A = F(rb0["allow"])
    edge = A
    for _ in range(64):
        if cr.stale(rb0["cut_now"], rb0["cut_list"], edge):
            break
        edge = np.nextafter(edge, INF)
    assert cr.stale(rb0["cut_now"], rb0["cut_list"], edge) and edge > A
    D = {"below": np.nextafter(A, F(0)), "at": A, "above": np.nextafter(A, INF), "edge_below": np.nextafter(edge, F(0)), "edge": edge,
         "nan": F(np.nan)}[where]
    moved = x2.copy()
    moved[3 * N_PT + K_MOVE, 0] = D
    assert bits(cr.disp_of(moved, x2)) == bits(D) or where == "nan"
    want = _moved_step(g, pairs, monkeypatch, x2, moved, rb0)
    assert want == (where in ("edge", "nan"))


def _ref_probability(em, d):
    s = Stats("ref")
    s.set_params(list(em))
    return float(s.prob_n(np.array([d], F))[0])


def test_staleness_is_not_vacuous(monkeypatch):
    """A left-out link, both ways.  Images 0 and 1, points 60 and 61, lie 0.25 mm beyond the list cutoff on the x axis.
    (i) Point 60's partner comes 0.4 mm closer, inside the allowance: the reference build still calls the link an outlier, the
    state stays 0, the list is in use and unchanged, and the sums have the bits of the full sweep.
    (ii) Point 61's partner comes to where the reference build calls the link an inlier.  A move just past the allowance
    cannot do that -- the cutoff sits where the probability is half the threshold, and 2 x 0.5 mm from cut + 1 mm is still behind
    it -- so the partner moves as far as it takes, far past the allowance: the state must be 1, and the sums have the bits of
    the full sweep, which they would not have if the flag had stayed down and the list had been swept."""
    need_ref()
    pairs, links = _edge_pairs()
    g, x2, rb0 = _built_thin(pairs, monkeypatch)
    g.close()
    cut = F(min(rb0["cut_list"][0], rb0["cut_list"][1]))
    far = F(cut + F(0.25))
    for k in (60, 61):
        x2[0 * N_PT + k] = (0.0, 0.0, 0.0)
        x2[1 * N_PT + k] = (far, 0.0, 0.0)
    row = {k: np.nonzero((links[:, 0] == k) & (links[:, 1] == N_PT + k))[0][0] for k in (60, 61)}

    def built():
        g = _deformable_group(pairs, monkeypatch, True, skin="1.0,1.0")
        g.set_points2(x2)
        g.updateDeformableTransforms(0.0)
        _, keep = _expected_listed(x2, links, rb0["cut_list"])
        assert not keep[row[60]] and not keep[row[61]]
        assert g.cull_stats()[:2] == (1, 2 * int(keep.sum()))
        return g
    # (i)
    g = built()
    moved = x2.copy()
    moved[N_PT + 60, 0] = F(far - F(0.4))
    d = float(np.sqrt(cr.link_d2(moved, [60], [N_PT + 60])[0]))
    assert min(_ref_probability(EM4[0], d), _ref_probability(EM4[1], d)) < 0.5
    assert not _moved_step(g, pairs, monkeypatch, x2, moved, rb0)
    # (ii)
    g = built()
    moved = x2.copy()
    d_in = next(d for d in np.arange(float(far), 0.0, -0.25) if min(_ref_probability(EM4[0], d), _ref_probability(EM4[1], d)) >= 0.5)
    moved[N_PT + 61, 0] = F(d_in)
    assert float(far) - d_in > 2.0 * float(rb0["allow"])
    full = _deformable_group(pairs, monkeypatch, False)
    full.set_points2(x2); full.updateDeformableTransforms(0.0)
    before = full.point_sums()
    assert _moved_step(g, pairs, monkeypatch, x2, moved, rb0)
    full.set_points2(moved); full.updateDeformableTransforms(0.0)
    after = full.point_sums()
    assert after[61, 3] > before[61, 3]                     # the link entered point 61's sums: a swept stale list would have missed it


# ---- (d) thin skins through every path that measures displacement ---------------------------------------------------------------

FORMS = {"pointwise": {"FROG_K11_POINTWISE": "1"}, "tiled": {"FROG_K11_TILED": "1"}, "neither": {}, "brick8": {"FROG_BRICK": "8"}}
SWITCHES = ("FROG_K11_POINTWISE", "FROG_K11_TILED", "FROG_BRICK", "FROG_SWEEP_FUSED", "FROG_CULL_SKIN", "FROG_CULL_BUILD_PASS",
            "FROG_WIDE_RECORDS")
ALPHA = {1: 0.3, 0: 0.02}           # with the guard on: large enough that it rejects steps (asserted)


class Probe:
    """An ImageGroup as a side of frog_amd.schedule that looks at the certificate before every deformable sweep."""

    def __init__(self, g, probe):
        self.g, self.probe, self.log = g, probe, []

    def __getattr__(self, name):
        return getattr(self.g, name)

    def updateDeformableTransforms(self, alpha):
        rb = self.g.cull_readback() if self.probe else None
        before = self.g.cull_stats()[0]
        e = self.g.updateDeformableTransforms(alpha)
        if rb:
            self.log.append((rb["state"], float(rb["disp_max"]), self.g.cull_stats()[0] - before))
        return e


def _stepped_schedule(pairs, monkeypatch, cull, skin, form, fused, gd):
    """_run_schedule (tests/gpu_util.py) with 10 linear iterations and 2 levels of 12, stepped through frog_amd.schedule's verbs."""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("FROG_CULL", "1" if cull else "0")
    if cull:
        monkeypatch.setenv("FROG_CULL_SKIN", skin)
    for name, value in FORMS[form].items():
        monkeypatch.setenv(name, value)
    if not fused:
        monkeypatch.setenv("FROG_SWEEP_FUSED", "0")
    side = Probe(ImageGroup(pairs, guarantee_diffeomorphism=gd), cull)
    E, rejected = [], [0]

    def on(tag, sides, e=None, infos=None):
        if schedule.kind(tag) in ("linear", "deformable"):
            E.append(float(np.float32(e[0])))           # the reference's Measure, a float: what ImageGroup.run keeps and _run_schedule compares
        elif schedule.kind(tag) == "step" and e[0] < 0:
            rejected[0] += 1
    grids = schedule.run([side], 10, [12, 12], alpha0=ALPHA[gd], on=on)
    g = side.g
    lattices = [[g.grid(i, k)[1].copy() for k in range(g.num_grids())] for i in range(pairs.n_images)]
    counts = [(c.inliers, c.outliers) for c in g.countInliers()]
    return dict(g=g, E=E, grids=grids, lattices=lattices, sums=g.point_sums().copy(), counts=counts, xyz2=g.points()[1].copy(),
                rejected=rejected[0], log=side.log)


@functools.lru_cache(maxsize=None)
def _group(name):
    return Pairs.synthetic(6, 3000, 1500, seed=7) if name == "small" else Pairs.synthetic(24, 400, 150, seed=5)


_FULL = {}
RUNS = [(skin, *rest) for skin in ("1.0,0.5", "1.0,2.0", "1.05,1.0")
        for rest in (("small", "pointwise", True, 1), ("many", "tiled", False, 0), ("small", "neither", False, 1), ("many", "brick8", True, 0))]


@pytest.mark.parametrize("skin,group,form,fused,gd", RUNS, ids=lambda v: str(v))
def test_thin_skin_schedule_is_bit_identical_to_the_full_sweep(monkeypatch, skin, group, form, fused, gd):
    """10 linear iterations and 2 levels of 12 deformable ones under skins of a millimetre, FROG_CULL=1 against FROG_CULL=0: energies
    (as the f32 the reference records; the two f64 sums behind them are re-associated by the compaction, k_cull.hip.h, and one ulp
    of f64 has been seen), lattices, per-point sums, census and coordinates bit-identical -- with the thread-per-point, the brick-of-8 and the tiled
    B-spline transform, each of which measures the displacement and raises the flag itself, with and without the fused sweep, with
    the diffeomorphism guard off and on (alpha 0.3: steps are rejected, the speculative coordinates of a rejected step are not
    published).  Both states of the certificate occur in every run: a sweep that walks the list after measured motion, a sweep
    that finds the flag raised by a transform, and 1 < builds < sweeps."""
    pairs = _group(group)
    key = (group, form, fused, gd)
    if key not in _FULL:
        r = _stepped_schedule(pairs, monkeypatch, False, None, form, fused, gd)
        r.pop("g").close()
        _FULL[key] = r
    full = _FULL[key]
    r = _stepped_schedule(pairs, monkeypatch, True, skin, form, fused, gd)
    assert r["grids"] == full["grids"] and r["rejected"] == full["rejected"]
    assert r["E"] == full["E"]
    for a, b in zip(r["lattices"], full["lattices"]):
        for x, y in zip(a, b):
            assert np.array_equal(bits(x), bits(y))
    assert np.array_equal(bits(r["sums"]), bits(full["sums"])) and r["counts"] == full["counts"]
    assert np.array_equal(bits(r["xyz2"]), bits(full["xyz2"]))
    if gd:
        assert r["rejected"] >= 1
    log = r["log"]
    sweeps, builds = len(log), r["g"].cull_stats()[0]
    # a sweep that found its list stale makes the next step rebuild: the list was in use where neither step built one
    in_use = sum(1 for (state, disp, built), (_, _, built_next) in zip(log, log[1:]) if state == 0 and disp > 0 and not built and not built_next)
    raised = sum(1 for state, disp, built in log if state == 1 and not built)
    note(f"thin_skin_{skin}_{group}_{form}_fused{int(fused)}_gd{gd}",
         f"builds {builds} sweeps {sweeps} list_in_use_after_motion {in_use} flag_raised_by_a_transform {raised} rejected {r['rejected']}")
    assert in_use >= 1 and raised >= 1 and 1 < builds < sweeps, (builds, sweeps, in_use, raised)
