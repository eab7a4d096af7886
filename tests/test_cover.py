"""frog_cover without a device (include/frog_chain.h): its NumPy restatement (cover_restate.py) against f64 statistics and
closed forms, the argument checks that come before the device is touched, and bin/AverageImage's flag errors."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from frog_amd import _abi
from frog_amd.chain import Link

import cover_restate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")
U = 2.0 ** -24                      # unit roundoff of float32


def _random_group(seed, n, dtype):
    """n sources of 6 x 7 x 8 at fractional affine maps over a 10 x 9 x 8 grid, masks of another geometry for two of them."""
    rng = np.random.default_rng(seed)
    grid = ((10, 9, 8), (-1.0, -0.5, 0.0), (1.0, 1.0, 1.0))
    images = []
    for k in range(n):
        M = np.eye(4)
        M[:3, :3] += rng.uniform(-0.05, 0.05, (3, 3))
        M[:3, 3] = rng.uniform(-3.0, 3.0, 3)
        vol = rng.uniform(-1000, 1000, (6, 7, 8)).astype(dtype)
        mask = None
        if k % 3 == 1:
            mask = (rng.integers(-1, 2, (5, 5, 5)).astype(np.int16), (0.0, 0.0, 0.0), (1.5, 1.5, 1.5))
        images.append(([Link.linear(M)], vol, (0.25, 0.0, -0.5), (1.0, 1.25, 0.75), mask))
    return images, grid


def test_restatement_against_f64_statistics():
    """Bound of the f32 update against the exact mean and population stdev of the valid values (u = 2^-24, M = max |x|, n
    images).  Step k computes d = x - mean, q = d / k, mean' = mean + q: three roundings, |d| <= 2M, |mean'| <= M, so the
    step adds at most (2 * 2M / k + M) u to the error of the mean, and an earlier error enters mean' with the factor
    1 - 1/k <= 1.  Summed over k <= n:  E = (n + 4 H_n) u M <= (n + 4 (1 + ln n)) u M.
    m2: d and e = x - mean' each carry the mean's error plus one rounding, E + 2M u, and are at most 2M, so the product
    carries 2 * 2M (E + 2M u) + 4M^2 u = 4M E + 12 M^2 u; the sum m2 <= 4M^2 k rounds by 4M^2 k u at step k.  After n steps
    and the division by n (one more rounding of a variance <= 4M^2):  V = 4M E + 12 M^2 u + 2 M^2 u (n + 1) + 4 M^2 u.
    stdev: |sqrt(a) - sqrt(b)| <= min(sqrt|a - b|, |a - b| / sqrt(b)), plus the rounding of the root, u * stdev.
    Terms of second order in u are left out: they are 1e-7 of the ones kept."""
    for seed, n, dtype in ((1, 6, "int16"), (2, 5, "float32"), (3, 2, "int16")):
        images, grid = _random_group(seed, n, dtype)
        mean, stdev, count = cover_restate.restate(images, grid)
        xs, vs = zip(*[cover_restate.terms(l, v, o, s, grid, m)[:2] for l, v, o, s, m in images])
        x = np.stack(xs).astype(np.float64)
        valid = np.stack(vs)
        k = valid.sum(0)
        assert np.array_equal(count, k) and count.dtype == np.uint16
        assert set(np.unique(k)) >= {0, 1, 2}
        safe = np.maximum(k, 1)
        exact_mean = np.where(valid, x, 0).sum(0) / safe
        exact_var = np.where(valid, (x - exact_mean) ** 2, 0).sum(0) / safe
        exact_sd = np.sqrt(exact_var)
        M = float(np.abs(x).max())
        E = (n + 4 * (1 + math.log(n))) * U * M
        V = 4 * M * E + 12 * M * M * U + 2 * M * M * U * (n + 1) + 4 * M * M * U
        covered = k > 0
        assert np.abs(mean[covered] - exact_mean[covered]).max() <= E
        with np.errstate(divide="ignore"):
            sd_bound = np.minimum(math.sqrt(V), V / exact_sd) + U * exact_sd
        assert (np.abs(stdev - exact_sd)[covered] <= sd_bound[covered]).all()
        assert (mean[~covered] == 0).all() and (stdev[~covered] == 0).all()
        assert not np.isnan(stdev).any() and (stdev[k == 1] == 0).all()
        # min_count and fill
        m2, s2, c2 = cover_restate.restate(images, grid, min_count=2, fill=-7.5)
        assert np.array_equal(c2, count)
        assert (m2[k < 2] == np.float32(-7.5)).all() and (s2[k < 2] == 0).all()
        assert np.array_equal(m2[k >= 2], mean[k >= 2]) and np.array_equal(s2[k >= 2], stdev[k >= 2])


def test_closed_forms():
    """Constant images: the first add gives d = c, mean = 0 + c / 1 = c, e = 0; every later one d = c - c = 0: the mean is c
    exactly and the stdev exactly 0.  Two values a, b: mean = a + (b - a) / 2, m2 = (b - a) * (b - mean) in float32."""
    shape = (3, 4, 5)
    for c in (0.1, -1024.0, 3.0e-41, 16777217.0):
        state = cover_restate.start(shape)
        x = np.full(shape, c, np.float32)
        for _ in range(7):
            state = cover_restate.update(state, x, np.ones(shape, bool))
        mean, stdev, count = cover_restate.finish(state)
        assert (mean == np.float32(c)).all() and (stdev == 0).all() and (count == 7).all()
    rng = np.random.default_rng(4)
    a = rng.normal(0, 1e3, shape).astype(np.float32)
    b = rng.normal(0, 1e3, shape).astype(np.float32)
    state = cover_restate.update(cover_restate.update(cover_restate.start(shape), a, np.ones(shape, bool)), b, np.ones(shape, bool))
    mean, stdev, count = cover_restate.finish(state)
    want = a + (b - a) / np.float32(2)
    assert want.dtype == np.float32 and np.array_equal(mean, want) and (count == 2).all()
    assert np.array_equal(stdev, np.sqrt(((b - a) * (b - want)) / np.float32(2)))
    # an image that is not valid leaves the voxel as it was
    valid = rng.random(shape) < 0.5
    state = cover_restate.update(cover_restate.update(cover_restate.start(shape), a, np.ones(shape, bool)), b, valid)
    mean, stdev, count = cover_restate.finish(state)
    assert np.array_equal(mean, np.where(valid, want, a)) and np.array_equal(count, 1 + valid)


def test_arguments_are_checked_before_the_device():
    """FROG_E_INVALID, never FROG_E_NODEVICE, whether or not a device is present."""
    lib = _abi.hip_lib()
    h = C.c_void_p()
    g = _abi.volume_view(None, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (4, 4, 4))
    assert lib.frog_cover_create(None, 0, C.byref(h)) == _abi.FROG_E_INVALID
    assert lib.frog_cover_create(C.byref(g), 0, None) == _abi.FROG_E_INVALID
    assert b"frog_cover_create" in lib.frog_last_error()
    g.dims[:] = (4, 0, 4)
    assert lib.frog_cover_create(C.byref(g), 0, C.byref(h)) == _abi.FROG_E_INVALID
    g.dims[:] = (2048, 1024, 1025)                              # 2^31 + 2^21 voxels
    assert lib.frog_cover_create(C.byref(g), 0, C.byref(h)) == _abi.FROG_E_INVALID
    assert b"2^31" in lib.frog_last_error()
    assert not h.value
    v = _abi.volume_view(np.zeros((4, 4, 4), np.int16), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    assert lib.frog_cover_add(None, None, C.byref(v), None, 1, 0.0, None) == _abi.FROG_E_INVALID
    assert lib.frog_cover_add(None, None, None, None, 1, 0.0, None) == _abi.FROG_E_INVALID
    out = np.zeros(64, np.float32)
    assert lib.frog_cover_finish(None, 1, 0.0, out.ctypes.data_as(_abi.c_float_p), None, None) == _abi.FROG_E_INVALID
    lib.frog_cover_destroy(None)
    if lib.frog_device_count() > 0:
        return                                                  # the NODEVICE answer is for hosts without a GPU
    g.dims[:] = (4, 4, 4)
    assert lib.frog_cover_create(C.byref(g), 0, C.byref(h)) == _abi.FROG_E_NODEVICE and not h.value


def test_average_image_flag_errors(tmp_path):
    exe = os.path.join(BIN, "AverageImage")

    def run(*args):
        return subprocess.run([exe, "bbox.json", "2", "a.nii.gz", "b.nii.gz", "c.nii.gz", "-o", "out", *args], cwd=tmp_path,
                              capture_output=True, text=True, timeout=60)

    r = subprocess.run([exe, "bbox.json", "2"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "[-c 1 [-ml masks.txt] [-mc minCount] [-f fill]]" in r.stdout
    (tmp_path / "two.txt").write_text("m0.nii.gz\nm1.nii.gz\n")
    for args in (("-mc", "2"), ("-f", "-1024"), ("-ml", "two.txt"), ("-mc", "2", "-c", "0")):
        r = run(*args)
        assert r.returncode == 1 and "need -c 1" in r.stdout, (args, r.stdout)
    r = run("-c", "1", "-ml", "two.txt")                        # N - 1 lines
    assert r.returncode == 1 and "two.txt holds 2 masks for 3 images" in r.stdout, r.stdout
    r = run("-c", "1", "-ml", "none.txt")
    assert r.returncode == 1 and "none.txt" in r.stdout, r.stdout
    r = run("-c", "1", "-mc", "0")
    assert r.returncode == 1 and "-mc" in r.stdout, r.stdout
    assert not (tmp_path / "out").exists()
