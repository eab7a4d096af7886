"""frog_labels without a device (include/frog_chain.h): the overlap identity the header states, and the argument checks of
frog_labels_create, which come before the device is touched."""
import ctypes as C

import numpy as np

from frog_amd import _abi

import labels_restate


def test_closed_form_is_the_pooled_pairwise_dice():
    """2 pairs / ((N - 1) voxels) from the vote counts equals the sum over all image pairs of 2 |A_i n A_j| over the sum of
    |A_i| + |A_j|, for every label of a random 5-image group.  Both sides are one f64 division of the same two integers
    (the closed form's numerator and denominator are the brute-force ones), so the comparison is exact."""
    rng = np.random.default_rng(17)
    base = rng.choice([0, 58, 86, 1247, -3], size=(6, 7, 8))
    vols = []
    for _ in range(5):
        v = base.copy()
        flip = rng.random(base.shape) < 0.3
        v[flip] = rng.choice([0, 58, 86, 1247, -3, 40358], size=int(flip.sum()))
        vols.append(v)
    r = labels_restate.restate(vols)
    n = len(vols)
    assert len(r["values"]) == 6 and r["values"][0] == -3
    closed = labels_restate.dice(r)
    for l, value in enumerate(r["values"]):
        masks = [v == value for v in vols]
        inter = sum(int((masks[i] & masks[j]).sum()) for i in range(n) for j in range(i + 1, n))
        sizes = sum(int(masks[i].sum()) + int(masks[j].sum()) for i in range(n) for j in range(i + 1, n))
        assert int(r["pairs"][l]) == inter and (n - 1) * int(r["voxels"][l]) == sizes
        assert closed[l] == labels_restate.brute_force_dice(vols, value)
        assert 0.0 < closed[l] < 1.0


def _create(dims, n_images, max_labels, grid=True, out=True):
    lib = _abi.hip_lib()
    g = _abi.volume_view(None, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), dims)
    h = C.c_void_p()
    rc = lib.frog_labels_create(C.byref(g) if grid else None, n_images, max_labels, 0, C.byref(h) if out else None)
    assert not h.value
    return rc


def test_create_validates_before_the_device():
    """FROG_E_INVALID, never FROG_E_NODEVICE, whether or not a device is present."""
    ok = (4, 4, 4)
    assert _create(ok, 0, 0) == _abi.FROG_E_INVALID
    assert _create(ok, 65536, 0) == _abi.FROG_E_INVALID
    assert _create(ok, 3, 65537) == _abi.FROG_E_INVALID
    assert _create((4, 0, 4), 3, 0) == _abi.FROG_E_INVALID
    assert _create((2048, 2048, 513), 3, 0) == _abi.FROG_E_INVALID        # above 2^31 voxels
    assert _create(ok, 3, 0, grid=False) == _abi.FROG_E_INVALID
    assert _create(ok, 3, 0, out=False) == _abi.FROG_E_INVALID
    assert b"frog_labels_create" in _abi.hip_lib().frog_last_error()
