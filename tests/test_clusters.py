"""Connected components and the cluster-extent test without a device: the restatement (clusters_restate.py) against
scipy.ndimage.label, cluster_p against its formula, and what frog_components and frog_clusters refuse before they ask for a
device.  Every comparison is == on integers or bits."""
import ctypes as C

import numpy as np
import pytest

from frog_amd import _abi
from frog_amd.volume import cluster_p

import clusters_restate as R

SHAPE = (23, 45, 67)                                        # z, y, x


def random_mask(density, seed, shape=SHAPE):
    return np.random.default_rng(seed).random(shape) < density


@pytest.mark.parametrize("density", [0.1, 0.3, 0.6])
@pytest.mark.parametrize("connectivity", [6, 18, 26])
def test_restatement_equals_scipy(connectivity, density):
    ndimage = pytest.importorskip("scipy.ndimage")
    mask = random_mask(density, int(density * 10) + connectivity)
    structure = ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity])
    want, n = ndimage.label(mask, structure)
    labels, count, largest = R.components(mask, connectivity)
    assert count == n and n >= 1 and (labels == want.astype(np.uint32)).all()
    assert n > 1 or density > 0.5                           # above the percolation threshold one component may take everything
    assert largest == np.bincount(want.reshape(-1))[1:].max()
    assert len(R.offsets(connectivity)) == connectivity


def test_restatement_on_designed_masks():
    empty = np.zeros((3, 4, 5), bool)
    assert R.components(empty)[1:] == (0, 0) and not R.components(empty)[0].any()
    assert R.components(~empty, 6)[1:] == (1, 60)
    # the roots are the smallest indices, the labels their ranks
    m = empty.copy()
    m[0, 0, 4] = m[0, 1, 0] = m[2, 3, 4] = m[2, 3, 3] = True
    labels, n, largest = R.components(m, 26)
    assert n == 3 and largest == 2 and labels[0, 0, 4] == 1 and labels[0, 1, 0] == 2 and labels[2, 3, 3] == labels[2, 3, 4] == 3


def test_cluster_p_follows_its_formula():
    rng = np.random.default_rng(5)
    null = rng.integers(0, 40, 200).astype(np.uint32)
    extent = np.concatenate([rng.integers(0, 45, 50), null[:5]]).astype(np.uint32)
    got = cluster_p(extent, null)
    assert got.dtype == np.float32 and got.shape == extent.shape
    for e, p in zip(extent, got):
        assert p == np.float32((1 + int((null[1:] >= e).sum())) / np.float64(200))
    # row 0 is the observed design and does not count; no null extent reaches the largest: 1 / n_perms
    assert cluster_p([41], np.array([100] + [40] * 9))[0] == np.float32(1 / np.float64(10))
    assert cluster_p([40], np.array([0] + [40] * 9))[0] == 1


def test_refusals_come_before_the_device_is_asked():
    """Each of these is FROG_E_INVALID also where there is no device.  What needs a live sink (another grid, permutations beyond
    the sink's, a slot out of range) is refused in tests/test_gpu_clusters.py."""
    lib = _abi.hip_lib()
    grid = _abi.volume_view(None, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (5, 4, 3))
    h = C.c_void_p()

    def create(g=C.byref(grid), k=4, c=2, two=0, t0=3.0, conn=26, out=C.byref(h)):
        return lib.frog_clusters_create(g, k, c, two, t0, conn, 0, out)

    empty = _abi.volume_view(None, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (5, 0, 3))
    for bad in (dict(g=None), dict(out=None), dict(g=C.byref(empty)), dict(k=0), dict(c=0), dict(c=_abi.FROG_GLM_MAX_CONTRASTS + 1), dict(t0=-0.5),
                dict(t0=float("nan")), dict(t0=float("inf")), dict(conn=0), dict(conn=8), dict(conn=27), dict(conn=-6)):
        assert create(**bad) == _abi.FROG_E_INVALID and not h.value, bad
    # frog_components
    voxels = np.ones((3, 4, 5), np.uint8)
    labels = np.empty((3, 4, 5), np.uint32)
    n, big = C.c_uint32(), C.c_uint64()

    def components(v=voxels, conn=26, lp=labels.ctypes.data_as(_abi.c_u32_p), np_=C.byref(n), bp=C.byref(big), null=False):
        view = _abi.volume_view(v, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
        return lib.frog_components(None if null else C.byref(view), conn, 0, lp, np_, bp)

    nodata = _abi.volume_view(voxels, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    nodata.data = None
    assert lib.frog_components(C.byref(nodata), 26, 0, labels.ctypes.data_as(_abi.c_u32_p), None, None) == _abi.FROG_E_INVALID
    for bad in (dict(null=True), dict(conn=4), dict(conn=19), dict(v=voxels.astype(np.float32)), dict(v=voxels.astype(np.float64)),
                dict(lp=None, np_=None, bp=None)):
        assert components(**bad) == _abi.FROG_E_INVALID, bad
    # a NULL sink
    f = (C.c_float * 4)()
    u = (C.c_uint32 * 4)()
    con = (C.c_double * 2)(0.0, 1.0)
    assert lib.frog_glm_permute_clusters(None, 1, con, 1, 0.0, None, 1, 1, u, None, 0, None, f, f) == _abi.FROG_E_INVALID
    assert lib.frog_clusters_finish(None, u) == _abi.FROG_E_INVALID
    assert lib.frog_clusters_mask(None, 0, 0, 0, (C.c_uint8 * 4)()) == _abi.FROG_E_INVALID
    assert lib.frog_clusters_labels(None, 0, 0, 0, u, None) == _abi.FROG_E_INVALID
    lib.frog_clusters_destroy(None)
