"""frog_staple without a device (include/frog_chain.h): the NumPy restatement (staple_restate.py) pinned on designed groups
-- where STAPLE repairs what majority vote gets wrong, the integer identities of the sums, the renormalisation that keeps a
600-image product from underflowing -- and the refusals of frog_amd.volume.Staple, which come before the device is touched."""
import numpy as np
import pytest

from frog_amd import _abi
from frog_amd.volume import Staple, staple_accuracy

import labels_restate
import staple_restate as sr


@pytest.fixture(scope="module")
def designed():
    truth, vols, R = sr.designed_group()
    return truth, vols, R, sr.restate(vols)


def test_staple_repairs_the_shared_mistake_of_majority_vote(designed):
    """Two exact maps and three with 30 % random errors that share label 2 in the 9 voxels of R, inside label 1: three
    mediocre maps outvote two good ones there, and STAPLE, which learns that they are mediocre, is right at every voxel."""
    truth, vols, R, r = designed
    assert all((v[R] == 2).all() for v in vols[2:]) and all((v[R] == 1).all() for v in vols[:2])
    assert list(r["values"]) == [0, 1, 2, 3]
    consensus = r["labels"].reshape(truth.shape)
    assert (consensus == truth).all()
    vote = labels_restate.restate(vols)["labels"]
    assert (vote[R] != truth[R]).all() and R.sum() == 9
    assert (vote != truth).sum() >= 9
    assert 0 < r["iterations"] < 50 and r["change"] < 1e-6
    sensitivity = sr.sensitivity(r).mean(1)
    assert sensitivity[:2].min() > sensitivity[2:].max()
    accuracy = staple_accuracy(r["sums"], r["totals"])
    assert accuracy[:2].min() > accuracy[2:].max() and np.argmin(accuracy) >= 2


def test_sums_are_integer_identities(designed):
    truth, vols, R, r = designed
    L = len(r["values"])
    for restrict in (False, True):
        x = r if not restrict else sr.restate(vols, restrict=True)
        assert x["sums"].dtype == np.uint64 and x["totals"].dtype == np.uint64
        for i in range(len(vols)):
            assert (x["sums"][i].sum(0, dtype=np.uint64) == x["totals"]).all()
        column = x["q"].astype(np.int64).sum(0)
        assert (np.abs(column - sr.ONE) <= L).all()
        assert x["prior"].sum() == pytest.approx(1.0, abs=1e-15)
    x = sr.restate(vols, restrict=True)
    stack = np.stack([v.ravel() for v in vols])
    unanimous = (stack == stack[0]).all(0)
    assert x["active_voxels"] == int((~unanimous).sum()) and 0 < x["active_voxels"] < truth.size
    assert (x["q"].max(0)[unanimous] == sr.ONE).all() and (x["q"].sum(0, dtype=np.int64)[unanimous] == sr.ONE).all()
    assert (x["q"][truth.ravel()[unanimous], np.flatnonzero(unanimous)] == sr.ONE).all()
    assert (x["labels"].reshape(truth.shape) == truth).all()                # restrict leaves the consensus unchanged
    assert (x["labels"] == r["labels"]).all()


def test_iteration_limits():
    truth, vols = sr.noisy_group(5, 0.3)
    zero = sr.restate(vols, max_iter=0)
    assert zero["iterations"] == 0 and zero["change"] == float("inf") and not zero["sums"].any() and not zero["totals"].any()
    assert (zero["theta"] == sr.start_theta(5, 4, 0.99)).all()
    one = sr.restate(vols, max_iter=1)
    assert one["iterations"] == 1 and np.isfinite(one["change"]) and (one["theta"] != zero["theta"]).any()
    assert ((one["q"] > 0) & (one["q"] < sr.ONE)).any(0).all()              # every voxel has a fractional q
    full = sr.restate(vols)
    assert 2 < full["iterations"] < 50 and full["change"] < 1e-6


def test_renormalisation_keeps_600_images_from_underflowing():
    """600 images with error rates from 0.7 x 35 % to 0.7 x 105 %, every error the next label: the plain f64 product of the
    first E-step's 600 factors is 0 at every voxel and label, the frexp steps return truth, and theta has entries below
    FLOOR (an image never shows two of the other labels), which the max(., FLOOR) of the E-step is there for."""
    rates = (0.35 + 0.70 * np.arange(600) / 599.0) * 0.7
    truth, vols = sr.noisy_group(600, rates, cyclic=True)
    r = sr.restate(vols)
    assert (r["labels"].reshape(truth.shape) == truth).all()
    assert (r["theta"] < sr.FLOOR).any()
    values, idx = sr.dense(vols)
    Da = np.stack(idx).astype(np.int64)
    start = sr.start_theta(600, 4, 0.99)
    assert (sr.e_step(Da, start, r["prior"], renormalise=False) == 0.0).all()      # the first E-step, at every voxel and label
    for theta in (start, r["theta"]):
        q = sr.e_step(Da, theta, r["prior"])
        assert (np.abs(q.astype(np.int64).sum(1) - sr.ONE) <= 4).all()


def test_single_label_and_unanimous_groups():
    one = sr.restate([np.full((2, 3, 4), 7, np.int16)] * 3)
    assert list(one["values"]) == [7] and (one["q"] == sr.ONE).all() and (one["theta"] == 1.0).all() and one["iterations"] == 2
    rng = np.random.default_rng(3)
    v = rng.choice([0, 58, 86], size=(2, 3, 4))
    same = sr.restate([v, v.copy(), v.copy()], restrict=True)
    assert same["active_voxels"] == 0 and same["iterations"] == 0 and same["change"] == float("inf")
    assert (same["labels"] == v.ravel()).all() and (same["confidence"] == 1.0).all() and not same["prior"].any()


def _invalid(call, *args):
    with pytest.raises(_abi.FrogError) as e:
        call(*args)
    assert e.value.code == _abi.FROG_E_INVALID, e.value
    return str(e.value)


def test_staple_refuses_bad_arguments_before_the_device():
    """FROG_E_INVALID, never FROG_E_NODEVICE, whether or not a device is present."""
    grid = ((4, 4, 4), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    assert "frog_staple_create" in _invalid(Staple, grid, 0)
    _invalid(Staple, grid, 4097)
    assert "256" in _invalid(Staple, grid, 3, 257)
    _invalid(Staple, ((4, 0, 4),) + grid[1:], 3)
    _invalid(Staple, ((2048, 2048, 513),) + grid[1:], 3)                   # above 2^31 voxels
    lib = _abi.hip_lib()
    import ctypes as C
    it, change, active = C.c_uint32(), C.c_double(), C.c_uint64()
    assert lib.frog_staple_solve(None, 0.99, 1e-6, 50, 0, C.byref(it), C.byref(change), C.byref(active)) == _abi.FROG_E_INVALID
    assert lib.frog_staple_performance(None, None, None, None, None) == _abi.FROG_E_INVALID
    from frog_amd import Staple as exported, staple_labels
    assert exported is Staple and callable(staple_labels)
