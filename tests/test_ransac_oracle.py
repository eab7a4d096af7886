"""RANSAC stage of the fixed-image mode (imageGroup.cxx:629-804): the oracle's restatement on cases with a
known answer.  VTK's vtkLandmarkTransform is absent (parity unpinned): what can be pinned is that the closed-form
similarity fit recovers a planted transform and that the census/selection rules hold."""
import numpy as np

import ransac_restate as rr
from frog_amd import _abi
from frog_amd.image_group import ransac_candidates
from frog_amd.pairs import Pairs
from oracle.oracle_api import OracleGroup


def planted_group(seed, n_points=400, outliers=0.3, noise=0.0):
    """Image 0 fixed; image 1 = inverse of a known similarity applied to image 0's points (+ false links)."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0, 200, (n_points, 3))
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    w, x, y, z = q
    R = np.array([[w*w+x*x-y*y-z*z, 2*(x*y-w*z), 2*(x*z+w*y)],
                  [2*(x*y+w*z), w*w-x*x+y*y-z*z, 2*(y*z-w*x)],
                  [2*(x*z-w*y), 2*(y*z+w*x), w*w-x*x-y*y+z*z]])
    s, t = 1.3, np.array([40.0, -25.0, 10.0])
    # moving point b with  a = s R b + t
    b = ((a - t) / s) @ R + rng.normal(0, noise, a.shape) if noise else ((a - t) / s) @ R
    po = np.array([0, n_points, 2 * n_points], np.uint32)
    xyz = np.concatenate([a, b]).astype(np.float32)
    n_false = int(outliers * n_points)
    p1 = np.concatenate([np.arange(n_points), rng.integers(0, n_points, n_false)]).astype(np.uint32)
    p2 = np.concatenate([np.arange(n_points), rng.integers(0, n_points, n_false)]).astype(np.uint32)
    order = np.argsort(p1, kind="stable")
    pairs = Pairs.from_arrays(po, xyz, [(0, 1, p1[order], p2[order])])
    M = np.eye(4); M[:3, :3] = s * R; M[:3, 3] = t
    return pairs, M, n_points


def prepared(pairs):
    ref = OracleGroup(pairs.model, _abi.FrogOptions.default(n_fixed_images=1))
    ref.setup_stats(); ref.linear_init(); ref.transform_points()
    return ref


def test_planted_similarity_is_recovered():
    pairs, M, n = planted_group(1)
    ref = prepared(pairs)
    best = ref.ransac(1, iterations=400, batches=4, inlier_distance=5.0)
    assert n <= best <= n + 5                      # every true link, at most a few false ones by chance
    assert np.allclose(ref.matrix(1), M, rtol=0, atol=2e-4)
    ref.transform_points()
    assert np.abs(ref.xyz2()[n:] - ref.xyz()[:n]).max() < 1e-3


def test_noise_is_averaged_by_the_refit():
    pairs, M, n = planted_group(2, noise=1.0)
    ref = prepared(pairs)
    ref.ransac(1, iterations=800, batches=8, inlier_distance=10.0)
    got = ref.matrix(1)
    # a 4-point candidate is off by the noise level; the refit over ~400 links is much closer
    assert np.abs(got[:3, :3] - M[:3, :3]).max() < 5e-3 and np.abs(got[:3, 3] - M[:3, 3]).max() < 1.0


def test_scale_filter_and_batch_split():
    pairs, M, n = planted_group(3)
    ref = prepared(pairs)
    before = ref.matrix(1).copy()
    # det = 1.3^3 = 2.197 > 2: every good candidate is refused; what remains has few inliers
    few = ref.ransac(1, iterations=200, batches=2, inlier_distance=5.0, max_scale=2.0)
    assert few < n // 4
    # iterations / batches rounds down (:636): 3 iterations in 4 batches = no candidate at all, matrix refitted
    # from the links the CURRENT matrix brings within the distance (none here -> identity, vtkLandmarkTransform)
    ref2 = prepared(pairs)
    assert ref2.ransac(1, iterations=3, batches=4, inlier_distance=1e-3) == 0
    assert np.array_equal(ref2.matrix(1), np.eye(4)) and not np.array_equal(before, np.eye(4))


def test_sparsely_linked_image_skips_the_same_candidates_as_the_product():
    """5 linked points (ransac_restate.sparse_group): about a fifth of the draws repeat correspondences until two distinct
    ones or fewer are left, a line.  Both sides refuse those (relative eigenvalue gap, similarity.h), so the oracle's best
    census is the selection rule's over the PRODUCT's candidates and flags with the restated counts, and its matrix is a
    similarity close to the planted one.  With the exact comparison of before, each side kept most of such draws with a
    rotation about the line of its own rounding."""
    pairs, planted = rr.sparse_group()
    ref = prepared(pairs)
    cand, usable = ransac_candidates(pairs, 1, iterations=400, batches=4, inlier_distance=2.0, max_scale=10.0)
    refused = (cand == np.eye(4)[:3].reshape(12)).all(axis=1)
    assert len(cand) == 400 and refused.sum() >= 50 and not usable[refused].any()
    owner, partner = rr.half_links(pairs, 1)
    counts = rr.census(cand, ref.xyz(), ref.xyz2(), owner, partner, 2.0)
    best, winner = rr.select(counts, usable, 4)
    assert ref.ransac(1, iterations=400, batches=4, inlier_distance=2.0) == best == 6
    m = ref.matrix(1)
    s2 = np.trace(m[:3, :3] @ m[:3, :3].T) / 3
    assert np.allclose(m[:3, :3] @ m[:3, :3].T, s2 * np.eye(3), rtol=0, atol=1e-12 * s2) and np.linalg.det(m[:3, :3]) > 0
    assert np.abs(m[:3, :3] - planted[:3, :3]).max() < 0.05 and np.abs(m[:3, 3] - planted[:3, 3]).max() < 2.0
