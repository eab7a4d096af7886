"""frog_jlabels without a device (include/frog_chain.h): the properties of its NumPy restatement (joint_restate.py) that the
device tests rely on -- the solve against an independent one, the normalisation, the designed cases, the validity rules --
and the argument checks that come before the device is touched."""
import math
import os
import subprocess
import sys

import numpy as np

import joint_restate
import wlabels_restate
from test_wlabels import SHAPE, designed_group

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


def random_group(n=6, seed=71):
    """(target, [image] x n): integer-valued float32 noise, the images mixed from the target and noise of their own."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 1000, SHAPE).astype(np.float32)
    images = [((1 - m) * t + m * rng.integers(0, 1000, SHAPE)).astype(np.float32) for m in np.linspace(0.1, 1.0, n)]
    return t, images


def full_matrices(K):
    """K[i][j] (j <= i) per voxel as (voxels, n, n) symmetric matrices."""
    n = len(K)
    out = np.empty(K[0][0].shape + (n, n), np.float64)
    for i in range(n):
        for j in range(i + 1):
            out[..., i, j] = out[..., j, i] = K[i][j]
    return out.reshape(-1, n, n)


def interior(shape, r):
    inside = np.zeros(shape, bool)
    inside[r:shape[0] - r, r:shape[1] - r, r:shape[2] - r] = True
    return inside


def test_the_solve_agrees_with_an_independent_one_and_the_weights_sum_to_one():
    """Raw weights against np.linalg.solve(K, 1): relative difference (largest entry's, over the largest weight) within
    n^2 cond(K) 2^-52, the worst case of a Cholesky-type factorisation.  The normalised weights, summed exactly
    (math.fsum), are 1 within n 2^-52."""
    t, images = random_group()
    every = np.ones(SHAPE, bool)
    n = len(images)
    for radius in (1, 2):
        jw = joint_restate.weights(t, every, [(a, every) for a in images], radius, 2, 0.1)
        K = full_matrices(jw["K"])
        raw = np.stack([w.ravel() for w in jw["raw"]], axis=1)
        norm = np.stack([w.ravel() for w in jw["norm"]], axis=1)
        want = np.linalg.solve(K, np.ones((len(K), n, 1)))[..., 0]
        cond = np.linalg.cond(K)
        relative = np.abs(raw - want).max(axis=1) / np.abs(want).max(axis=1)
        assert (relative <= n * n * cond * EPS).all(), (relative / (n * n * cond * EPS)).max()
        sums = np.array([math.fsum(row) for row in norm])
        assert (np.abs(sums - 1.0) <= n * EPS).all(), np.abs(sums - 1.0).max() / EPS
        assert all(w.dtype == np.float32 for w in jw["w"])


def test_an_affine_copy_of_the_target_gets_the_largest_weight():
    """2 t + 5 has the target's normalised patch up to the rounding of the two means, so its d is a few ulps where the two
    patches cover the same voxels: its row of M all but vanishes and it takes the largest weight at every interior voxel.  A
    flat target normalises to zeros, every d_i is |A^_i|: M_ii is the patch's voxel count, and no weight is NaN or inf."""
    t, match, n1, n2 = designed_group()
    every = np.ones(SHAPE, bool)
    rng = np.random.default_rng(7)
    images = [n1, match, n2, rng.integers(0, 1000, SHAPE).astype(np.float32)]
    for radius in (1, 2):
        M = joint_restate.gram(t, every, [(a, every) for a in images], radius)
        assert M[1][1].max() <= 1e-24 and M[0][0].min() > 1
        jw = joint_restate.weights(t, every, [(a, every) for a in images], radius, 2, 0.1)
        inside = interior(SHAPE, radius)
        assert inside.any()
        for k in (0, 2, 3):
            assert (jw["w"][1][inside] > jw["w"][k][inside]).all()
        assert (jw["w"][1] > 0.9).all()
        flat = np.full(SHAPE, 7, np.float32)
        M = joint_restate.gram(flat, every, [(a, every) for a in images], radius)
        count = (2 * radius + 1) ** 3
        assert np.allclose(M[0][0][inside], count, rtol=1e-9, atol=0)
        jw = joint_restate.weights(flat, every, [(a, every) for a in images], radius, 2, 0.1)
        assert all(np.isfinite(w).all() for w in jw["w"]) and all(np.isfinite(w).all() for w in jw["raw"])


REGION = (slice(2, 10), slice(2, 12), slice(2, 14))         # of a 12 x 14 x 16 grid (z, y, x)
REGION_INTERIOR = (slice(4, 8), slice(4, 10), slice(4, 12))     # its voxels whose radius-2 patch lies inside it
RADIUS = 2


def correlated_group():
    """The case the method exists for.  Target: noise.  Atlases 0 and 1 are the target plus small noise of their own and
    carry label 1 everywhere.  Atlases 2, 3 and 4 add one shared error image E inside REGION (and small noise of their
    own) and carry label 2 there: three atlases that are wrong in the same way."""
    rng = np.random.default_rng(11)
    shape = (12, 14, 16)
    t = rng.integers(0, 1000, shape).astype(np.float32)
    E = np.zeros(shape)
    E[REGION] = rng.normal(0, 100, shape)[REGION]
    atlases = []
    for k in range(5):
        image = t + rng.normal(0, 30, shape) + (E if k >= 2 else 0)
        labels = np.full(shape, 1, np.uint8)
        if k >= 2:
            labels[REGION] = 2
        atlases.append((np.rint(image).astype(np.float32), labels))
    return t, atlases


def test_three_atlases_with_one_shared_error_outvote_two_good_ones_only_without_the_joint_solve():
    t, atlases = correlated_group()
    voted = wlabels_restate.restate(t, atlases, RADIUS, 2, 2.0 ** -10)
    joint = joint_restate.restate(t, atlases, RADIUS, 2, 0.1)
    assert voted["labels"][REGION_INTERIOR].size == 4 * 6 * 8
    assert (voted["labels"][REGION_INTERIOR] == 2).all()
    assert (joint["labels"][REGION_INTERIOR] == 1).all()
    outside = np.ones(t.shape, bool)
    outside[REGION] = False
    assert (joint["labels"][outside] == 1).all() and (voted["labels"][outside] == 1).all()
    # the three share one vote: together they weigh less than either good atlas
    shared = sum(w.astype(np.float64) for w in joint["weights"][2:])
    assert (shared[REGION_INTERIOR] < np.minimum(joint["weights"][0], joint["weights"][1])[REGION_INTERIOR]).all()


def test_validity_rules_and_the_restricted_system():
    """No valid target or no active atlas: the fill label, confidence 0, probability 0.  An atlas that is not valid at v has
    weight 0 there and the others' weights sum to 1; their bits are those of the header's solve on K restricted to them."""
    t, images = random_group(5, seed=73)
    rng = np.random.default_rng(79)
    t = t.copy()
    t[3, 6, 9] = np.nan
    images = [a.copy() for a in images]
    for a in images:
        a[2, 3, 4] = np.inf                                     # no active atlas
    images[1][4, 5, 6] = np.nan
    images[1][4, 5, 7] = np.nan
    images[3][4, 5, 7] = np.nan
    images[0][1, 1, 1] = images[2][1, 1, 1] = images[3][1, 1, 1] = images[4][1, 1, 1] = np.nan     # one active atlas
    atlases = [(a, rng.choice([0, 58, 86], size=SHAPE).astype(np.int16)) for a in images]
    r = joint_restate.restate(t, atlases, 1, 2, 0.1, fill_label=-7)
    for v in ((3, 6, 9), (2, 3, 4)):
        assert r["labels"][v] == -7 and r["confidence"][v] == 0 and r["total"][v] == 0
        assert all(joint_restate.probability(r, value)[v] == 0 for value in r["values"])
        assert all(w[v] == 0 for w in r["weights"])
    assert r["weights"][1][1, 1, 1] == 1 and all(r["weights"][k][1, 1, 1] == 0 for k in (0, 2, 3, 4))
    tt, valid_t = joint_restate.staged(t)
    staged = [joint_restate.staged(a) for a in images]
    jw = joint_restate.weights(tt, valid_t, staged, 1, 2, 0.1)
    for v, out in (((4, 5, 6), [1]), ((4, 5, 7), [1, 3]), ((1, 1, 1), [0, 2, 3, 4]), ((5, 5, 5), [])):
        keep = [i for i in range(5) if i not in out]
        assert [bool(jw["active"][i][v]) for i in range(5)] == [i in keep for i in range(5)]
        assert all(jw["norm"][i][v] == 0 and jw["w"][i][v] == 0 for i in out)
        assert abs(math.fsum(float(jw["norm"][i][v]) for i in keep) - 1.0) <= 5 * EPS
        K = [[float(jw["K"][max(i, j)][min(i, j)][v]) for j in keep] for i in keep]
        raw, norm = joint_restate.solve_literal(K)
        assert raw == [float(jw["raw"][i][v]) for i in keep] and norm == [float(jw["norm"][i][v]) for i in keep]


CHILD = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from frog_amd import _abi
lib = _abi.hip_lib()
def create(dims=(4, 4, 4), n=3, max_labels=0, radius=2, beta=2, alpha=0.1, keep=0, grid=True, out=True):
    g = _abi.volume_view(None, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), dims)
    h = C.c_void_p()
    rc = lib.frog_jlabels_create(C.byref(g) if grid else None, n, max_labels, radius, beta, alpha, keep, 0, C.byref(h) if out else None)
    assert not h.value
    return rc
bad = [create(n=0), create(n=33), create(max_labels=65537), create(radius=0), create(radius=4), create(beta=0), create(beta=5),
       create(alpha=0.0), create(alpha=-0.1), create(alpha=float("nan")), create(alpha=float("inf")), create(dims=(4, 0, 4)),
       create(dims=(2048, 2048, 513)), create(grid=False), create(out=False)]
assert bad == [_abi.FROG_E_INVALID] * len(bad), bad
v = _abi.volume_view(None, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (4, 4, 4))
n = C.c_uint32()
null = [lib.frog_jlabels_target(None, None, C.byref(v), 1, 0.0, None), lib.frog_jlabels_add(None, None, C.byref(v), C.byref(v), 1, 0.0, 0.0, None, None),
        lib.frog_jlabels_finish(None, C.byref(n)), lib.frog_jlabels_values(None, None), lib.frog_jlabels_fused(None, 0, None, None),
        lib.frog_jlabels_probability(None, 0, None), lib.frog_jlabels_weight(None, 0, None)]
assert null == [_abi.FROG_E_INVALID] * len(null), null
lib.frog_jlabels_destroy(None)
print("refused", len(bad) + len(null))
"""


def test_arguments_are_refused_before_the_device_is_touched():
    """FROG_E_INVALID, never FROG_E_NODEVICE, in a child process that is shown no device."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "refused 22" in r.stdout, r.stdout + r.stderr
