"""The scatter's phase 2 accumulates a point's 64 x 4 products with one f32 matrix instruction (k_grid.hip.h scatter_accumulate:
v_mfma_f32_4x4x1_16b_f32, K = 1, i.e. fmaf per element).  Two checks that it has the bits of the per-lane fmaf form:

  the accumulate step alone   frog_test_scatter_accumulate runs one wavefront over n points by the kernel's helper and by an fmaf
                              loop per lane; inputs in which every lane and every register carries its own value, so that a wrong
                              fragment layout (operands swapped, rows for columns) cannot agree;
  the kernel                  designed groups (tests/scatter_cases.py) through the default library and through the build whose
                              phase 2 is a plain fmaf loop (-DFROG_SCATTER_QUADS=0, `make variants`), in two processes: proposal
                              lattices, energies and coordinates of three steps, bit for bit.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import lattice_design as ld
import scatter_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
VARIANT = os.path.join(os.path.dirname(HERE), "frog_amd", "lib", "variants", "libfrog_hip_noquads.so")


# ---- the accumulate step alone ---------------------------------------------------------------------------------------------

def accumulate(sums, weights, start, plain):
    """frog_test_scatter_accumulate: sums [n, 4], weights [n, 64], start [64, 4] -> [64, 4] (tap, component)."""
    from frog_amd import _abi
    sums = np.ascontiguousarray(sums, np.float32); weights = np.ascontiguousarray(weights, np.float32)
    start = np.ascontiguousarray(start, np.float32)
    n = len(sums)
    assert sums.shape == (n, 4) and weights.shape == (n, 64) and start.shape == (64, 4)
    out = np.full((64, 4), np.nan, np.float32)
    p = lambda a: a.ctypes.data_as(_abi.c_float_p)
    _abi.check(_abi.hip_lib().frog_test_scatter_accumulate(0, p(sums), p(weights), n, p(start), p(out), int(plain)),
               "frog_test_scatter_accumulate")
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def both(sums, weights, start):
    got, want = accumulate(sums, weights, start, False), accumulate(sums, weights, start, True)
    differ = np.argwhere(bits(got) != bits(want))
    assert len(differ) == 0, (len(differ), differ[:4].tolist(), got[tuple(differ[0])], want[tuple(differ[0])])
    return got


def distinct(n, seed):
    """Every sum, weight and starting value its own: no two lanes, registers or points share a value, signs mixed."""
    rng = np.random.default_rng(seed)
    sums = rng.permutation(4 * n).reshape(n, 4) / 7.0 + 0.5
    weights = (rng.permutation(64 * n).reshape(n, 64) + 1.0) / 61.0
    start = rng.permutation(256).reshape(64, 4) * 3.0 - 300.0
    sums[rng.random((n, 4)) < 0.5] *= -1.0
    return sums.astype(np.float32), weights.astype(np.float32), start.astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 4, 5, 64])
def test_accumulate_distinct_values(n):
    """n = 1, 3, 4, 5, 64 points (64: a chain of 64 dependent updates on every accumulator).  The two modes agree bit for bit,
    and the result is the rank-1 update it should be: within 2^-23 n of sum |w s| + |start| of the f64 sum, which rows taken for
    columns or swapped operands miss by far (every value is distinct and of order 1 to 100)."""
    sums, weights, start = distinct(n, seed=n)
    got = both(sums, weights, start)
    s, w, r = sums.astype(np.float64), weights.astype(np.float64), start.astype(np.float64)
    want = r + np.einsum("qt,qc->tc", w, s)
    scale = np.abs(r) + np.einsum("qt,qc->tc", np.abs(w), np.abs(s))
    assert np.all(np.abs(got - want) <= 2.0 ** -23 * n * scale)
    # with the operands exchanged, register r of lane 4 b + j would hold w[4 b + r] s[j]: far outside that bar, which therefore
    # tells the layouts apart
    swapped = r + np.einsum("qbr,qj->bjr", w.reshape(n, 16, 4), s).reshape(64, 4)
    assert np.count_nonzero(np.abs(swapped - want) > 2.0 ** -23 * n * scale) >= 128


def _special(name):
    t = np.arange(64, dtype=np.float64)
    c = np.arange(4, dtype=np.float64)
    tc = 4.0 * t[:, None] + c[None, :]                       # 0..255, one per (lane, register)
    if name == "subnormal":
        # products 2^-146 .. 2^-127 (subnormal, most inexact), a subnormal sum (3 x 2^-140) times weights of order 1,
        # starting values that are subnormal themselves; 5 points
        n = 5
        q = np.arange(n, dtype=np.float64)[:, None]
        sums = np.concatenate([2.0 ** -76 * (1 + q / 128), 3 * 2.0 ** -140 * (1 + q), -2.0 ** -64 * (1 + q / 32), 2.0 ** -57 * (1 + q / 8)],
                              axis=1)
        weights = np.where(t[None, :] < 32, 2.0 ** -70 * (1 + t[None, :] / 64), 0.5 + t[None, :] / 128) * (1 + q / 1024)
        start = (tc - 100.0) * 2.0 ** -149
        return sums, weights, start, None
    if name == "cancel":
        # start = -(w s) exactly (small integers and halves): every sum is an exact zero, and x + (-x) is +0
        sums = np.array([[1.0, -2.0, 3.0, -0.5]])
        weights = (t + 1.0)[None, :]
        start = -weights[0][:, None] * sums[0][None, :]
        return sums, weights, start, np.zeros((64, 4), np.float32)
    if name == "minus_zero":
        # a weight of -0 in the even lanes, +0 in the odd ones, start -0: the sum is -0 where the product is -0 (weight and sum
        # of unlike sign), +0 where it is +0
        sums = np.array([[1.5, -2.5, 1e-30, -1e30]])
        weights = np.where(t % 2 == 0, -0.0, 0.0)[None, :]
        start = np.full((64, 4), -0.0)
        want = np.where((t[:, None] % 2 == 0) == (sums[0][None, :] > 0), -0.0, 0.0).astype(np.float32)
        return sums, weights, start, want
    if name == "overflow":
        # products and starting values in the last two binades; the sums stay finite in lanes below 48 and overflow to
        # +-inf in the others
        sums = np.array([[2.0 ** 63, -2.0 ** 63, 1.5 * 2.0 ** 62, 2.0 ** 63 * (1 + 2.0 ** -23)]])
        weights = (2.0 ** 63 * (1 + t / 64))[None, :]
        big = np.where(t[:, None] < 48, 2.0 ** 126, 1.9 * 2.0 ** 127) * (1 + tc / 1024)
        start = big * np.sign(sums[0])[None, :]
        return sums, weights, start, None
    raise KeyError(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["subnormal", "cancel", "minus_zero", "overflow"])
def test_accumulate_special_values(name):
    """Subnormal products, sums and accumulators (not flushed); exact cancellation to +0; a -0 weight; the last binades below
    overflow and beyond.  Both modes agree bit for bit; where IEEE arithmetic fixes the result outright it is that result."""
    sums, weights, start, want = _special(name)
    with np.errstate(over="ignore"):
        sums, weights, start = sums.astype(np.float32), weights.astype(np.float32), start.astype(np.float32)
    got = both(sums, weights, start)
    if want is not None:
        assert np.array_equal(bits(got), bits(want))
    if name == "subnormal":
        tiny = np.abs(got) < 2.0 ** -126
        assert np.count_nonzero(tiny & (got != 0)) >= 64          # subnormal results are there, and are not flushed
        # registers 0 and 1 of lanes >= 32 add a subnormal product to a subnormal start: exact in f64
        want = start.astype(np.float64)
        for q in range(len(sums)):
            want = (want + weights[q].astype(np.float64)[:, None] * sums[q].astype(np.float64)[None, :]).astype(np.float32).astype(np.float64)
        assert np.array_equal(got[32:, 1], want[32:, 1].astype(np.float32))
    if name == "overflow":
        assert np.all(np.isfinite(got[:48])) and np.all(np.isinf(got[48:]))


# ---- the kernel on designed geometry -------------------------------------------------------------------------------------------

# (no gpu mark, on purpose: numpy only, it checks the fixtures and runs with the CPU suite)
def test_the_groups_are_what_they_are_designed_to_be():
    """The block sizes, runs and holes the cases are named after, counted with numpy (lattice_design.brick_of)."""
    lat = ld.Lattice.level(0)
    po, xyz, blocks, linked = sc.build("sizes")
    for image in range(3):
        x = xyz[po[image]:po[image + 1]]
        b = ld.brick_of(x, lat, 4)
        for brick, want in sc.SIZES.items():
            assert int(np.count_nonzero(np.all(b == np.array(brick), axis=1))) == want, (image, brick)
        assert np.array_equal(ld.cells32(x, lat)[0], ld.cells32(xyz[:po[1]], lat)[0])     # the copies lie in image 0's cells
    assert set(sc.SIZES.values()) == {1, 3, 4, 5, 63, 64, 65, 384, 385}
    po, xyz, blocks, linked = sc.build("cells")
    x = xyz[:po[1]]
    cell = ld.cells32(x, lat)[0]
    b = ld.brick_of(x, lat, 4)
    own = np.all(b == 1, axis=1)
    assert np.count_nonzero(own) == 64 and len(np.unique(cell[own], axis=0)) == 64
    one = np.all(b == np.array([1, 0, 0]), axis=1)
    assert np.count_nonzero(one) == sc.ONE_CELL[1] > 128 and len(np.unique(cell[one], axis=0)) == 1
    two = np.all(b == np.array([0, 1, 0]), axis=1)
    _, per_cell = np.unique(cell[two], axis=0, return_counts=True)
    assert sorted(per_cell) == [30, 70]
    holes = np.all(b == np.array([0, 0, 1]), axis=1)
    assert np.count_nonzero(holes) == 90 and np.count_nonzero(holes & ~linked) == 30 and np.all(linked[~holes][2:])
    po, xyz, blocks, linked = sc.build("stray")
    box = ld.Lattice([9] * 3, [0.0] * 3, [8.0] * 3)
    for image in range(3):
        assert np.count_nonzero(ld.stray(xyz[po[image]:po[image + 1]], box, 4) & linked) == 1


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The cases through both builds: {False: default library, True: the point-by-point build}, each an .npz."""
    if not os.path.exists(VARIANT):
        pytest.skip("frog_amd/lib/variants/libfrog_hip_noquads.so not built (make -C frog_amd/csrc variants)")
    tmp = tmp_path_factory.mktemp("scatter_mfma")
    out = {}
    for plain in (False, True):
        env = dict(os.environ)
        env.pop("FROG_HIP_LIB", None)
        for name in ("FROG_BRICK", "FROG_REFERENCE_ORDER", "FROG_ENERGY_PASS"):
            env.pop(name, None)
        if plain:
            env["FROG_HIP_LIB"] = "variants/libfrog_hip_noquads.so"
        path = tmp / ("plain.npz" if plain else "product.npz")
        r = subprocess.run([sys.executable, os.path.join(HERE, "run_scatter_cases.py"), str(path)], env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out[plain] = np.load(path)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(sc.CASES))
def test_kernel_equals_the_fmaf_build_bit_for_bit(runs, case):
    """One step and a schedule of three: proposal lattices (frog_get_grid), energies and coordinates after every step, equal bit
    for bit between the matrix-instruction build and the per-lane fmaf build.  The cases: scatter blocks of 1, 3, 4, 5, 63, 64,
    65, 384 and 385 points; a block whose points share one cell; one with a cell change at every point; batches that begin
    inside a cell's run; unlinked points in the middle of a batch; one stray point per image; and all of it with bricks of 8^3
    cells (the 11^3 tile)."""
    a, b = runs[False], runs[True]
    keys = sorted(k for k in a.files if k.startswith(case + "/"))
    assert keys == sorted(k for k in b.files if k.startswith(case + "/")) and len(keys) == 3 + 3 * sc.STEPS
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert a[k].tobytes() == b[k].tobytes(), k
    # the run did what the case is about
    group, brick, box = sc.CASES[case]
    po, xyz, blocks, linked = sc.build(group)
    assert int(a[f"{case}/strays"]) == (3 * sc.STEPS if group == "stray" else 0)
    sums = a[f"{case}/sums"]
    assert np.array_equal(sums[:, 3] != 0, np.tile(linked, 3)) and set(np.unique(sums[:, 3])) == {0.0, 2.0}
    assert list(a[f"{case}/dims"]) == ([9] * 3 if box else [15] * 3)
    for step in range(sc.STEPS):
        lattice = a[f"{case}/lattice{step}"]
        assert np.all(np.isfinite(lattice)) and all(np.any(lattice[i]) for i in range(3))
        assert np.isfinite(a[f"{case}/E{step}"]) and a[f"{case}/E{step}"] > 0
    assert np.any(a[f"{case}/xyz2_0"] != xyz) and np.any(a[f"{case}/xyz2_2"] != a[f"{case}/xyz2_0"])
