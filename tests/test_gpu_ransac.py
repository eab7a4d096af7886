"""The RANSAC stage piece by piece (frog_ransac: candidates, census, selection and refit).

The census of EVERY candidate, through frog_test_ransac_census -- frog_ransac's own launch --, against tests/ransac_restate.py
with == on the whole array, on groups designed for the kernel's edges: the last partial wavefront of an image, a thread's 8
half-links, a block's 2048, the flush of the parked counts every 64 candidates and at the end of the list, points without
links (ties in the binary search for a half-link's owner), the threshold itself.  Then frog_ransac's census and matrix against
the selection rule written out in ransac_restate.select and the refit of tests/similarity_util.py on the winner's inlier
half-links."""
import numpy as np
import pytest

import ransac_restate as rr
import similarity_util as su
from frog_amd import _abi
from frog_amd.image_group import ImageGroup, ransac_candidates
from frog_amd.pairs import Pairs
from oracle.oracle_api import OracleGroup

pytestmark = pytest.mark.gpu

F4, F8 = np.float32, np.float64
N_CANDIDATES = (1, 63, 64, 65, 127, 128, 129, 600)


def started(pairs, xyz2=None, **options):
    g = ImageGroup(pairs, **options)
    g.setupLinearTransforms()
    g.transformPoints()
    if xyz2 is not None:
        g.set_points2(xyz2)
    return g


def degrees_for(n_links, rng):
    """Points with 0..3 links each, n_links in all."""
    d = []
    while sum(d) < n_links:
        d.append(min(int(rng.integers(0, 4)), n_links - sum(d)))
    return d


def sliding_candidates(n, xyz, xyz2, owner, partner, distance, rng):
    """n distinct matrices whose counts differ: xyz2 is laid out so that half-link l sits u_l = (l + 0.5) W / L further
    along x than its own point, and candidate c is a small rotation about the centroid with a translation that brings the
    links with u_l < (c + 1) W / n (more with every candidate) within the distance.  Returns (candidates, xyz2)."""
    L, W = len(owner), 0.5 * distance
    xyz2 = np.array(xyz2, F4)
    u = (np.arange(L) + 0.5) * W / L
    xyz2[partner] = xyz[owner] + np.stack([u, np.zeros(L), np.zeros(L)], axis=1).astype(F4)   # a shared partner keeps the last
    cand = np.zeros((n, 3, 4))
    centre = xyz[owner].astype(F8).mean(axis=0)
    for c in range(n):
        q = np.concatenate([[1.0], rng.normal(0, 2e-4, 3)])
        R = rr.quaternion_matrix(q)
        cand[c, :, :3] = R
        cand[c, :, 3] = centre - R @ centre + [(c + 1) * W / n - distance, rng.normal(0, 0.01), rng.normal(0, 0.01)]
    return cand.reshape(n, 12), xyz2


def check_census(g, pairs, image, cand, distance, xyz2=None):
    xyz, read_back = g.points()
    assert np.array_equal(xyz, pairs.xyz)
    if xyz2 is not None:
        assert np.array_equal(read_back, xyz2)
    owner, partner = rr.half_links(pairs, image)
    want = rr.census(cand, xyz, read_back, owner, partner, distance)
    for n in [k for k in N_CANDIDATES if k <= len(cand)] + [len(cand)]:
        got = g.ransac_census(image, cand[:n], distance)
        assert got.dtype == np.uint32 and np.array_equal(got, want[:n]), (n, np.flatnonzero(got != want[:n])[:8])
    return want


@pytest.mark.parametrize("n_links", [1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 5003])
def test_census_of_every_candidate(n_links):
    """1 .. 600 candidates (prefixes of one list of distinct matrices with rising counts) over an image whose half-links
    end inside a wavefront, at its end and one past it; the same for a wavefront's 8 x 64 and a block's 256 x 8."""
    rng = np.random.default_rng(n_links)
    pairs = rr.designed_group(degrees_for(n_links, rng), image=1, n_partner=max(37, 2 * n_links), seed=n_links)
    owner, partner = rr.half_links(pairs, 1)
    assert len(owner) == n_links
    g = started(pairs)
    cand, xyz2 = sliding_candidates(600, np.array(pairs.xyz), g.points()[1], owner, partner, 5.0, rng)
    g.set_points2(xyz2)
    want = check_census(g, pairs, 1, cand, 5.0, xyz2)
    assert len(np.unique(want)) >= min(600, n_links) // 2 + 1 and want.max() >= (n_links + 1) // 2   # the counts do differ


EMPTY_ROWS = {
    "first": lambda d: [0] + d,
    "last": lambda d: d + [0],
    "run": lambda d: d[:20] + [0] * 9 + d[20:],
    "all_but_one": lambda d: [0] * 30 + [7] + [0] * 30,
}


@pytest.mark.parametrize("image", [0, 1, 2])
@pytest.mark.parametrize("where", sorted(EMPTY_ROWS))
def test_points_without_links(where, image):
    """Runs of equal row pointers are ties in the kernel's search for a half-link's owner; with the measured image first,
    in the middle and last in the group the image's first point is row 0 or a later one."""
    rng = np.random.default_rng(7)
    degrees = EMPTY_ROWS[where]([int(k) for k in rng.integers(1, 4, 45)])
    pairs = rr.designed_group(degrees, image=image, n_partner=400, seed=3)
    owner, partner = rr.half_links(pairs, image)
    g = started(pairs)
    cand, xyz2 = sliding_candidates(70, np.array(pairs.xyz), g.points()[1], owner, partner, 5.0, rng)
    g.set_points2(xyz2)         # a half-link given to a neighbouring row would be measured from another point, far away
    want = check_census(g, pairs, image, cand, 5.0, xyz2)
    assert want.max() >= len(owner) // 2 and len(np.unique(want)) > min(20, len(owner) // 2)


def test_duplicate_links_count_once_per_copy():
    rng = np.random.default_rng(8)
    degrees = degrees_for(150, rng)
    once, thrice = (rr.designed_group(degrees, n_partner=300, seed=4, duplicate=k) for k in (1, 3))
    owner, partner = rr.half_links(once, 1)
    assert len(rr.half_links(thrice, 1)[0]) == 3 * len(owner) == 450
    g1, g3 = started(once), started(thrice)
    cand, xyz2 = sliding_candidates(65, np.array(once.xyz), g1.points()[1], owner, partner, 5.0, rng)
    g1.set_points2(xyz2); g3.set_points2(xyz2)
    want = check_census(g1, once, 1, cand, 5.0, xyz2)
    assert np.array_equal(check_census(g3, thrice, 1, cand, 5.0, xyz2), 3 * want) and want.max() > 70


def test_threshold_is_strict_and_overflows_to_every_link():
    """inlier_distance 5, integer coordinates, a pure translation: the link at exactly (3, 4, 0) has d2 == 25 and is out;
    one float32 step closer it is in, one further out.  A distance whose square overflows float32 lets every finite
    distance in."""
    a = np.array([[10, 20, 30], [-7, 14, 2], [40, -33, 8]], F4)
    t = np.array([100.0, -50.0, 25.0])
    at = (a.astype(F8) + t).astype(F4)
    step = np.array([np.nextafter(F4(at[1, 0] + 3), F4(0)) - at[1, 0], 4, 0], F4)      # (3 - one step at 113, 4, 0)
    step_out = np.array([np.nextafter(F4(at[2, 0] + 3), F4(1e9)) - at[2, 0], 4, 0], F4)
    b = np.stack([at[0] + F4([3, 4, 0]), at[1] + step, at[2] + step_out]).astype(F4)
    assert step[0] < 3 < step_out[0] and np.array_equal(b[1] - at[1], step)
    pairs = Pairs.from_arrays([0, 3, 6], np.concatenate([b, a]), [(0, 1, [0, 1, 2, 2], [0, 1, 2, 2])])
    g = started(pairs, xyz2=np.array(pairs.xyz), n_fixed_images=1)
    shift = np.concatenate([np.eye(3), t[:, None]], axis=1).reshape(12)
    far = shift.copy(); far[3] = 1e30
    cand = np.stack([shift, far])
    assert np.array_equal(check_census(g, pairs, 1, cand, 5.0), [1, 0])
    assert np.array_equal(check_census(g, pairs, 1, cand, 5.0000005), [2, 0])          # the next float32: 25.000004
    assert np.array_equal(check_census(g, pairs, 1, cand, 1e20), [4, 0])               # inf: all, but not inf < inf


def test_non_finite_candidates_count_nothing_and_disturb_nobody():
    rng = np.random.default_rng(9)
    pairs = rr.designed_group(degrees_for(700, rng), n_partner=1400, seed=5)
    owner, partner = rr.half_links(pairs, 1)
    g = started(pairs)
    cand, xyz2 = sliding_candidates(130, np.array(pairs.xyz), g.points()[1], owner, partner, 5.0, rng)
    g.set_points2(xyz2)
    clean = rr.census(cand, np.array(pairs.xyz), xyz2, owner, partner, 5.0)
    bad = {5: (0, np.nan), 63: (3, np.inf), 64: (7, -np.inf), 70: (10, np.nan), 129: (11, np.inf)}
    for c, (entry, value) in bad.items():
        cand[c, entry] = value
    want = check_census(g, pairs, 1, cand, 5.0, xyz2)
    assert all(want[c] == 0 for c in bad) and clean.min() > 0
    keep = np.setdiff1d(np.arange(130), list(bad))
    assert np.array_equal(want[keep], clean[keep])


def test_partners_are_the_fixed_images_transformed_positions():
    """With fixed images the census is taken against THEIR xyz2 (where their transforms put them), not their xyz."""
    rng = np.random.default_rng(10)
    pairs = rr.designed_group(degrees_for(300, rng), image=2, n_images=3, n_partner=600, seed=6)
    owner, partner = rr.half_links(pairs, 2)
    g = started(pairs, n_fixed_images=2)
    cand, xyz2 = sliding_candidates(65, np.array(pairs.xyz), g.points()[1], owner, partner, 5.0, rng)
    before = check_census(g, pairs, 2, cand, 5.0)                   # as transformPoints left the table
    g.set_points2(xyz2)
    after = check_census(g, pairs, 2, cand, 5.0, xyz2)
    assert not np.array_equal(before, after) and after.max() > 150


# ---- selection and refit ----------------------------------------------------------------------------------------------------
T_A = rr.similarity((0.8, 0.1, 0.5, -0.2), 1.3, (40.0, -25.0, 10.0))
T_B = rr.similarity((0.3, -0.7, 0.2, 0.6), 0.9, (-60.0, 35.0, 80.0))


def two_cluster_group():
    """12 points that follow T_A and 12 that follow T_B: a draw inside one cluster fits its 12 half-links and none of the
    other's, so candidates of the two kinds tie at 12 with different inlier sets; mixed draws fit next to nothing."""
    moving = np.random.default_rng(11).uniform(-90, 90, (24, 3))
    return rr.planted_group(moving, [T_A, T_B], [0] * 12 + [1] * 12)


def reference_refit(src, tgt, start):
    """(matrix, bound) of the least-squares similarity through the correspondences as similarity.h states it: the identity
    for none, a translation for one, `start` (the candidate is kept) for two or an undetermined rotation, else the fit: at 60
    digits if mpmath is there, through the SVD if not."""
    if len(src) < 2:
        m = np.eye(4)
        if len(src):
            m[:3, 3] = tgt[0].astype(F8) - src[0].astype(F8)
        return m, 0.0
    relgap, mag = su.relgap_f64(src, tgt)
    if len(src) == 2 or not relgap > su.tau():
        assert len(src) == 2 or not relgap > su.tau() / 1024          # the designed cases are nowhere near the threshold
        return start, 0.0
    assert relgap > su.tau() * 1024
    try:
        import mpmath                                               # noqa: F401
    except ImportError:
        return su.kabsch_svd(src, tgt), su.error_bound(relgap, mag, su.K + su.K_SVD)
    ref, relgap, mag = su.horn_mp(src, tgt)
    return np.array([[float(v) for v in row] for row in ref]), su.error_bound(relgap, mag)


def run_and_check(pairs, image, xyz2=None, **options):
    """frog_ransac against the pieces: its census is the rule's value over the restated counts of its own candidates, its
    matrix the reference refit on the winner's inlier half-links (the current matrix's when nobody wins; the winner itself
    when the refit is refused).  Returns what the case-specific assertions need."""
    o = dict(iterations=200, batches=4, inlier_distance=5.0, max_scale=10.0)
    o.update(options)
    g = started(pairs, xyz2=xyz2, n_fixed_images=image)
    xyz, read_back = g.points()
    owner, partner = rr.half_links(pairs, image)
    cand, usable = ransac_candidates(pairs, image, **o)
    assert len(cand) == o["iterations"] // o["batches"] * o["batches"]
    counts = rr.census(cand, xyz, read_back, owner, partner, o["inlier_distance"])
    assert np.array_equal(g.ransac_census(image, cand, o["inlier_distance"]), counts)
    # the flags: a refused fit leaves the identity; |det| as a float against the bounds
    det = np.abs(np.linalg.det(cand.reshape(-1, 3, 4)[:, :, :3])).astype(F4)
    refused = (cand == np.eye(4)[:3].reshape(12)).all(axis=1)
    flags = ~refused & ~(det > F4(o["max_scale"])) & ~(det.astype(F8) < 1.0 / F8(F4(o["max_scale"])))
    assert np.array_equal(usable, flags)
    best, winner = rr.select(counts, usable, o["batches"])
    current = g.matrix(image).copy()
    assert g.RANSAC(image, **o) == best
    start = np.concatenate([cand[winner].reshape(3, 4), [[0, 0, 0, 1]]]) if winner >= 0 else current
    inl = rr.inliers(start[:3].reshape(12), xyz, read_back, owner, partner, o["inlier_distance"])
    assert winner < 0 or inl.sum() == best
    return dict(g=g, cand=cand, usable=usable, counts=counts, best=best, winner=winner, start=start, inl=inl,
                src=xyz[owner[inl]], tgt=read_back[partner[inl]], owner=owner, partner=partner, xyz=xyz, xyz2=read_back, options=o)


def assert_refit(r, image):
    ref, bound = reference_refit(r["src"], r["tgt"], r["start"])
    got = r["g"].matrix(image)
    assert np.abs(got - ref).max() <= bound, (np.abs(got - ref).max(), bound)


def test_ties_inside_a_batch_and_between_batches():
    pairs = two_cluster_group()
    r = run_and_check(pairs, 1)
    assert r["best"] == 12
    per = len(r["cand"]) // 4
    tied = np.flatnonzero(r["usable"] & (r["counts"] == 12))
    sets = {c: tuple(rr.inliers(r["cand"][c], r["xyz"], r["xyz2"], r["owner"], r["partner"], 5.0)) for c in tied}
    other = [c for c in tied if sets[c] != sets[r["winner"]]]
    assert r["winner"] == tied[0] and r["winner"] < per
    assert any(c < per for c in other) and any(c >= per for c in other)      # a tie of each kind, with another answer
    assert_refit(r, 1)
    planted = T_A if r["inl"][0] else T_B
    assert np.abs(r["g"].matrix(1) - planted).max() < 1e-4


@pytest.mark.parametrize("inverse", [False, True])
def test_determinant_just_inside_and_outside_the_scale_bounds(inverse):
    """|det| = 1.3^3 (or its inverse) against max_scale a thousandth above and below it."""
    T = np.linalg.inv(T_A) if inverse else T_A
    moving = np.random.default_rng(12).uniform(-90, 90, (20, 3))
    pairs = rr.planted_group(moving, [T], [0] * 20)
    inside = run_and_check(pairs, 1, max_scale=1.3 ** 3 * 1.001)
    assert inside["best"] == 20 and inside["usable"].sum() > 100
    assert_refit(inside, 1)
    outside = run_and_check(pairs, 1, max_scale=1.3 ** 3 * 0.999)
    good = outside["counts"] == 20
    assert good.sum() > 100 and not outside["usable"][good].any() and outside["best"] < 20
    assert_refit(outside, 1)


def test_no_usable_candidate_refits_from_the_current_matrix():
    moving = np.random.default_rng(13).uniform(-90, 90, (20, 3))
    pairs = rr.planted_group(moving, [rr.similarity((1, 0, 0, 0), 1.3, (1.0, -2.0, 0.5))], [0] * 20)
    r = run_and_check(pairs, 1, max_scale=1.0000001, inlier_distance=30.0)
    assert not r["usable"].any() and r["best"] == 0 and r["winner"] == -1
    assert 3 <= r["inl"].sum() < 20                                 # what the current matrix brings within the distance
    assert_refit(r, 1)


def test_winner_with_collinear_inliers_is_kept_as_it_is():
    """10 points on a line and 10 off it, all following one transform in the fixed image's xyz, which the draws read; in
    xyz2, which the census reads, the partners of the points off the line are far away.  A draw with a point off the line
    gives the exact transform, its inliers are the 10 on the line: the refit is refused and the candidate stays."""
    rng = np.random.default_rng(14)
    line = np.array([5.0, -20.0, 11.0]) + np.arange(-5, 5)[:, None] * np.array([6.0, 2.0, -3.0])
    moving = np.concatenate([line, rng.uniform(-90, 90, (10, 3))])
    pairs = rr.planted_group(moving, [T_A], [0] * 20)
    xyz2 = np.array(pairs.xyz)
    xyz2[10:20] += 1000.0
    r = run_and_check(pairs, 1, xyz2=xyz2)
    assert r["best"] == 10 and r["inl"][:10].all() and not r["inl"][10:].any()
    assert np.array_equal(r["g"].matrix(1), r["start"])


def test_sparsely_linked_image():
    """5 linked points: about a fifth of the draws hold two distinct correspondences or fewer.  Before similarity_fit compared the
    eigenvalues relatively, most of those were accepted with the rotation about their line that rounding had left, fitted
    their two points exactly and competed on the census; the oracle's Jacobi variant rounds differently, so the two sides
    disagreed about which candidates existed and, when such a candidate won, about the matrix."""
    pairs, planted = rr.sparse_group()
    r = run_and_check(pairs, 1, iterations=400, inlier_distance=2.0)
    refused = ~r["usable"] & (r["cand"] == np.eye(4)[:3].reshape(12)).all(axis=1)
    assert refused.sum() >= len(r["cand"]) // 8 and len(np.unique(r["counts"][r["usable"]])) >= 3
    assert_refit(r, 1)
    m = r["g"].matrix(1)
    s2 = np.trace(m[:3, :3] @ m[:3, :3].T) / 3
    assert np.allclose(m[:3, :3] @ m[:3, :3].T, s2 * np.eye(3), rtol=0, atol=1e-12 * s2) and np.linalg.det(m[:3, :3]) > 0
    ref = OracleGroup(pairs.model, _abi.FrogOptions.default(n_fixed_images=1))
    ref.setup_stats(); ref.linear_init(); ref.transform_points()
    assert ref.ransac(1, **r["options"]) == r["best"]
    assert np.allclose(m, ref.matrix(1), rtol=1e-9, atol=1e-9)
    again = started(pairs, n_fixed_images=1)
    assert again.RANSAC(1, **r["options"]) == r["best"] and np.array_equal(again.matrix(1), m)
