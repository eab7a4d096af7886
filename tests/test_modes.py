"""The principal modes of a group without a device: the NumPy restatement (modes_restate.py) against plain float64 PCA on the
designed case, frog_modes_eigen (host code) against numpy.linalg, and the restatement's windows.

The designed case: 12 images on a 13 x 11 x 9 grid, 3 components; field_i = mean + sum_k B_ik sd_k psi_k with three
orthogonal planted modes psi of rms 1 per value, sd = 4, 2, 1 mm, B centred with orthogonal columns of norm sqrt(11), values
stored as float32.  Eigenvalue k is then sd_k^2 x values, mode k is sd_k psi_k and the scores are B, up to the float32 store.
Bars: modes within 2^-21 x the largest stored magnitude (8 rounding units of the store); eigenvalues within 2^-21 relative;
scores within 2^-21 of the column's largest magnitude; the fourth rms below 2^-21 x the first."""
import numpy as np
import pytest

from frog_amd import _abi
from frog_amd.volume import modes_eigen

import modes_restate as R

F8 = np.float64
BAR = 2.0 ** -21


def pack(G):
    return np.asarray(G, F8)[np.tril_indices(len(G))]


def designed_solution():
    """The restatement's pipeline on the designed case: (eigenvalues, vectors, mean, modes, n_support, fields)."""
    fields = R.designed_case()[0]
    n = len(fields)
    g, n_support = R.gram(fields)
    values, vectors = modes_eigen(g, n - 1)
    mean, modes = R.project(fields, vectors[:4] / np.sqrt(F8(n - 1)))
    return values, vectors, mean, modes, n_support, fields


def check_designed(values, vectors, mean, modes, n_support, fields, report=print):
    """Test 1's bars, on any solution of the designed case (the device's, in test_gpu_modes)."""
    _, planted_mean, psi, B = R.designed_case()
    n, count = len(fields), fields[0].size
    assert n_support * 3 == count
    want_values, want_modes, want_scores = R.plain_pca(fields)
    largest = float(np.abs(fields).max())
    rms = np.sqrt(np.maximum(values, 0) / count)
    scores = np.sqrt(F8(n - 1)) * vectors.T
    figures = dict(eigen=float(np.max(np.abs(values[:3] - want_values[:3]) / want_values[:3])),
                   modes=float(np.abs(modes[:3].reshape(3, -1) - want_modes[:3]).max()),
                   scores=float(np.max(np.abs(scores[:, :3] - want_scores[:, :3]).max(axis=0) / np.abs(want_scores[:, :3]).max(axis=0))),
                   mean=float(np.abs(mean.reshape(-1) - np.asarray(fields, F8).reshape(n, -1).mean(axis=0)).max()),
                   fourth=float(rms[3] / rms[0]), largest=largest)
    report(figures)
    assert figures["eigen"] <= BAR and figures["modes"] <= BAR * largest and figures["scores"] <= BAR and figures["fourth"] < BAR
    assert figures["mean"] <= BAR * largest
    # and plain PCA finds what was planted: the rms per value, the modes and the scores
    sign = np.where(B[np.argmax(np.abs(B), axis=0), np.arange(3)] < 0, -1.0, 1.0)
    assert np.abs(rms[:3] / np.array(R.DESIGNED_SD) - 1).max() <= BAR
    assert np.abs(modes[:3].reshape(3, -1) - (sign * np.array(R.DESIGNED_SD))[:, None] * psi).max() <= BAR * largest
    assert np.abs(scores[:, :3] - B * sign).max() <= BAR * np.abs(B).max()
    return figures


def test_restatement_recovers_the_designed_case():
    figures = check_designed(*designed_solution())
    assert 9 < figures["largest"] < 30


def eigen_cases():
    rng = np.random.default_rng(11)

    def spd(n):
        A = rng.normal(size=(n, n + 3))
        return A @ A.T

    low = rng.normal(size=(12, 3))
    cases = {"designed": R.unpack(R.gram(R.designed_case()[0])[0]) / 11.0}
    for n in (2, 3, 17, 64):
        cases[f"random{n}"] = spd(n)
    cases.update(rank3=low @ low.T, identity2=2.0 * np.eye(5), zero=np.zeros((4, 4)), huge=spd(6) * 1e150, tiny=spd(6) * 1e-150)
    return cases


@pytest.mark.parametrize("name", list(eigen_cases()))
def test_eigen_against_numpy(name):
    G = eigen_cases()[name]
    G = (G + G.T) / 2
    n = len(G)
    values, vectors = modes_eigen(pack(G))
    E = vectors.T                                           # columns
    trace = float(np.trace(G))
    bar = n * 2.0 ** -50
    want = np.linalg.eigvalsh(G)[::-1]
    assert (np.diff(values) <= 0).all()
    assert np.abs(values - want).max() <= bar * trace
    scale = max(float(np.linalg.norm(G)), np.finfo(F8).tiny)
    assert np.linalg.norm(G - (E * values) @ E.T) <= bar * scale if trace > 0 else (values == 0).all()
    assert np.linalg.norm(E.T @ E - np.eye(n)) <= bar * np.sqrt(n)
    for k in range(n):
        at = int(np.argmax(np.abs(vectors[k])))
        assert vectors[k, at] > 0 and abs(np.linalg.norm(vectors[k]) - 1) <= 2.0 ** -50
    # eigenvectors one by one, where the gap to the neighbours exceeds a thousandth of the trace
    w, V = np.linalg.eigh(G)
    V = R.sign_rule(V.T[::-1])
    gaps = np.abs(np.diff(want))
    compared = 0
    for k in range(n):
        gap = min([gaps[j] for j in (k - 1, k) if 0 <= j < n - 1] or [np.inf])
        if trace > 0 and gap > trace / 1000:
            compared += 1
            assert np.abs(vectors[k] - V[k]).max() <= bar * trace / gap * 8, k
    assert compared or name in ("identity2", "zero")


def test_eigen_orders_ties_and_refuses():
    values, vectors = modes_eigen(pack(2.0 * np.eye(4)))
    assert (values == 2).all() and (vectors == np.eye(4)).all()            # ties keep index order
    values, vectors = modes_eigen(pack(np.diag([1.0, 3.0, 1.0, 3.0])), 2.0)
    assert (values == [1.5, 1.5, 0.5, 0.5]).all() and (vectors == np.eye(4)[[1, 3, 0, 2]]).all()
    lib = _abi.hip_lib()
    out = np.empty(16, F8).ctypes.data_as(_abi.c_double_p)
    g = np.ones(3, F8)
    gp = g.ctypes.data_as(_abi.c_double_p)
    assert lib.frog_modes_eigen(2, gp, 1.0, out, out) == _abi.FROG_OK
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.frog_modes_eigen(2, gp, bad, out, out) == _abi.FROG_E_INVALID, bad
    assert lib.frog_modes_eigen(0, gp, 1.0, out, out) == _abi.FROG_E_INVALID
    assert lib.frog_modes_eigen(_abi.FROG_MODES_MAX_IMAGES + 1, gp, 1.0, out, out) == _abi.FROG_E_INVALID
    assert lib.frog_modes_eigen(2, None, 1.0, out, out) == _abi.FROG_E_INVALID and lib.frog_modes_eigen(2, gp, 1.0, None, out) == _abi.FROG_E_INVALID
    for bad in (float("nan"), float("inf")):
        g[1] = bad
        assert lib.frog_modes_eigen(2, gp, 1.0, out, out) == _abi.FROG_E_INVALID, bad


def test_create_and_planes_refuse_before_the_device_is_touched():
    """Every refusal of the grid, the window, the image count and the component count comes before the first HIP call: the
    code is FROG_E_INVALID with or without a device."""
    import ctypes as C
    lib = _abi.hip_lib()
    h, planes = C.c_void_p(), C.c_uint32()

    def grid(dims):
        return C.byref(_abi.volume_view(None, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), dims))

    good = (5, 4, 3)
    for dims, first, count, n, comps in ((good, 0, 3, 1, 3), (good, 0, 3, _abi.FROG_MODES_MAX_IMAGES + 1, 3), (good, 0, 3, 4, 2), (good, 0, 3, 4, 0),
                                         (good, 0, 0, 4, 3), (good, 3, 1, 4, 3), (good, 1, 3, 4, 3), ((5, 0, 3), 0, 3, 4, 3),
                                         ((1 << 11, 1 << 10, (1 << 10) + 1), 0, 1, 4, 1)):
        assert lib.frog_modes_create(grid(dims), first, count, n, comps, 0, C.byref(h)) == _abi.FROG_E_INVALID, (dims, first, count, n, comps)
    assert lib.frog_modes_create(None, 0, 3, 4, 3, 0, C.byref(h)) == _abi.FROG_E_INVALID
    assert lib.frog_modes_create(grid(good), 0, 3, 4, 3, 0, None) == _abi.FROG_E_INVALID
    for n, comps in ((1, 3), (_abi.FROG_MODES_MAX_IMAGES + 1, 1), (4, 2)):
        assert lib.frog_modes_planes(grid(good), n, comps, 0, C.byref(planes)) == _abi.FROG_E_INVALID
    assert lib.frog_modes_planes(grid(good), 4, 3, 0, None) == _abi.FROG_E_INVALID
    f = np.empty(8, np.float32).ctypes.data_as(_abi.c_float_p)
    d = np.zeros(8, F8).ctypes.data_as(_abi.c_double_p)
    assert lib.frog_modes_plane(None, 0, f) == _abi.FROG_E_INVALID
    assert lib.frog_modes_gram(None, None, d, C.byref(C.c_uint64())) == _abi.FROG_E_INVALID
    assert lib.frog_modes_project(None, None, 1, d, 0.0, f, f) == _abi.FROG_E_INVALID
    assert lib.frog_modes_add_displacement(None, None, None, None) == _abi.FROG_E_INVALID
    assert lib.frog_modes_add_jacobian(None, None, None, None, 0) == _abi.FROG_E_INVALID
    assert lib.frog_modes_add(None, None, None, None, 1, 0.0) == _abi.FROG_E_INVALID


def window_case():
    """7 images, 3 components on a 37 x 21 x 5 grid (2331 values per plane: three chunks, the last short), one image with holes,
    a region with holes and one plane outside the support."""
    rng = np.random.default_rng(3)
    planes = rng.normal(0, 3, (7, 5, 21, 37, 3)).astype(np.float32)
    holes = rng.random((5, 21, 37)) < 0.1
    planes[2][holes] = R.NAN
    region = (rng.random((5, 21, 37)) < 0.9).astype(np.uint8)
    region[3] = 0
    return planes, region


def test_windows_in_the_restatement():
    planes, region = window_case()
    whole, support = R.gram(planes, region)
    assert support == int(R.support(planes, region).sum()) and 0 < support < region.sum()
    for cuts in ([1] * 5, [2, 1, 2]):
        g, s, at = None, 0, 0
        for m in cuts:
            g, s = R.gram(planes[:, at:at + m], region[at:at + m], g, s)
            at += m
        assert g.tobytes() == whole.tobytes() and s == support
    # the order of the windows matters: descending order gives other bits
    g, s = None, 0
    for z in reversed(range(5)):
        g, s = R.gram(planes[:, z:z + 1], region[z:z + 1], g, s)
    assert s == support and g.tobytes() != whole.tobytes() and np.allclose(g, whole, rtol=1e-12)
    w = np.random.default_rng(4).normal(size=(3, 7))
    mean, modes = R.project(planes, w, region, -2.0)
    parts = [R.project(planes[:, z:z + 1], w, region[z:z + 1], -2.0) for z in range(5)]
    assert np.concatenate([p[0] for p in parts]).tobytes() == mean.tobytes()
    assert np.concatenate([p[1] for p in parts], axis=1).tobytes() == modes.tobytes()
    assert (mean[3] == -2).all() and (modes[:, 3] == -2).all()
