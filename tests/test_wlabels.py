"""frog_wlabels without a device (include/frog_chain.h): the properties of its NumPy restatement (wlabels_restate.py) that the
device tests' designed cases rely on, its bridge to the majority vote, and the argument checks that come before the device is
touched."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

from frog_amd import _abi

import labels_restate
import wlabels_restate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (7, 13, 19)


def designed_group():
    """(target, matching, noise1, noise2): integer-valued float32 noise as the target, 2 t + 5, and two independent noise
    images, on the 19 x 13 x 7 grid."""
    rng = np.random.default_rng(5)
    t = rng.integers(0, 1000, SHAPE).astype(np.float32)
    n1 = rng.integers(0, 1000, SHAPE).astype(np.float32)
    n2 = rng.integers(0, 1000, SHAPE).astype(np.float32)
    return t, (2 * t + 5).astype(np.float32), n1, n2


def test_an_affine_copy_of_the_target_weighs_one_and_noise_little():
    t, match, n1, n2 = designed_group()
    every = np.ones(SHAPE, bool)
    for radius, bound in ((1, 0.44), (2, 0.16)):
        w, member = wlabels_restate.weights(t, every, match, every, radius, 2, 2.0 ** -10)
        assert member.all() and w.dtype == np.float32 and (w == 1.0).all()
        for noise in (n1, n2):
            w, _ = wlabels_restate.weights(t, every, noise, every, radius, 2, 2.0 ** -10)
            assert 0 < w.max() <= bound and w.min() >= np.float32(2.0 ** -20)


def test_a_constant_target_leaves_the_floor():
    _, _, n1, _ = designed_group()
    every = np.ones(SHAPE, bool)
    flat = np.full(SHAPE, 7, np.float32)
    for floor, power in ((2.0 ** -10, 2), (0.25, 3), (0.0, 1)):
        w, _ = wlabels_restate.weights(flat, every, n1, every, 1, power, floor)
        assert (w == np.float32(floor) ** power).all()
    r = wlabels_restate.restate(flat, [(n1, np.full(SHAPE, 58, np.uint8))], 1, 2, 0.0, fill_label=-7)
    assert (r["total"] == 0).all() and (r["labels"] == -7).all() and (r["confidence"] == 0).all()
    assert (wlabels_restate.probability(r, 58) == 0).all()


def test_non_members_neither_vote_nor_enter_a_patch():
    """A NaN in the atlas takes the voxel out of the 27 patches around it, and only there: elsewhere the weights are those
    of the clean atlas; the voxel itself gets no vote."""
    t, match, _, _ = designed_group()
    every = np.ones(SHAPE, bool)
    holed = match.copy()
    holed[3, 6, 9] = np.nan
    clean = wlabels_restate.restate(t, [(match, np.ones(SHAPE, np.uint8))], 1, 1, 0.0)
    r = wlabels_restate.restate(t, [(holed, np.ones(SHAPE, np.uint8))], 1, 1, 0.0)
    assert r["total"][3, 6, 9] == 0 and r["labels"][3, 6, 9] == 0
    far = np.ones(SHAPE, bool)
    far[2:5, 5:8, 8:11] = False
    assert np.array_equal(r["total"][far], clean["total"][far])
    near = ~far
    near[3, 6, 9] = False
    assert (r["total"][near] == 1.0).all()               # 26 exact members of an exact line still correlate perfectly


def test_floor_one_is_the_majority_vote():
    """With floor = 1 every weight is 1, the scores are the vote counts: fused map, confidence (= agreement) and
    probabilities of labels_restate on a group with unanimous, all-different, 3-3 and 2-2-2 slabs."""
    rng = np.random.default_rng(23)
    pool = [0, 58, 86, 170, 1247, 29193, 40358]
    vols = [rng.choice(pool, size=SHAPE) for _ in range(6)]
    for k, (v, value) in enumerate(zip(vols, (170, -3, 40358, 29193, 1247, 86))):
        v[0] = 58
        v[1] = value
        v[2] = 86 if k < 3 else 58
        v[3] = (86, 1247, 0)[k // 2]
    images = [rng.integers(0, 1000, SHAPE).astype(np.float32) for _ in vols]
    t = rng.integers(0, 1000, SHAPE).astype(np.float32)
    want = labels_restate.restate(vols)
    got = wlabels_restate.restate(t, list(zip(images, vols)), 2, 3, 1.0)
    assert np.array_equal(got["values"], want["values"])
    assert np.array_equal(got["scores"], want["counts"].astype(np.float32))
    assert np.array_equal(got["labels"], want["labels"])
    assert got["confidence"].dtype == np.float32 and np.array_equal(got["confidence"], want["agreement"])
    for value in want["values"]:
        assert np.array_equal(wlabels_restate.probability(got, value), labels_restate.probability(want, value))


CHILD = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from frog_amd import _abi
lib = _abi.hip_lib()
def create(dims=(4, 4, 4), n=3, max_labels=0, radius=2, power=2, floor=0.5, grid=True, out=True):
    g = _abi.volume_view(None, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), dims)
    h = C.c_void_p()
    rc = lib.frog_wlabels_create(C.byref(g) if grid else None, n, max_labels, radius, power, floor, 0, C.byref(h) if out else None)
    assert not h.value
    return rc
bad = [create(n=0), create(max_labels=65537), create(radius=0), create(radius=5), create(power=0), create(power=9),
       create(floor=-0.001), create(floor=1.001), create(floor=float("nan")), create(dims=(4, 0, 4)), create(dims=(2048, 2048, 513)),
       create(grid=False), create(out=False)]
assert bad == [_abi.FROG_E_INVALID] * len(bad), bad
v = _abi.volume_view(None, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (4, 4, 4))
n = C.c_uint32()
null = [lib.frog_wlabels_target(None, None, C.byref(v), 1, 0.0, None), lib.frog_wlabels_add(None, None, C.byref(v), C.byref(v), 1, 0.0, 0.0, None, None),
        lib.frog_wlabels_finish(None, C.byref(n)), lib.frog_wlabels_values(None, None), lib.frog_wlabels_fused(None, 0, None, None),
        lib.frog_wlabels_probability(None, 0, None)]
assert null == [_abi.FROG_E_INVALID] * len(null), null
lib.frog_wlabels_destroy(None)
print("refused", len(bad) + len(null))
"""


def test_arguments_are_refused_before_the_device_is_touched():
    """FROG_E_INVALID, never FROG_E_NODEVICE, in a child process that is shown no device."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "refused 19" in r.stdout, r.stdout + r.stderr
