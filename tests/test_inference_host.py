"""The inference of GroupStats' permutation test as the tool's header states it (frog_amd/csrc/host/inference.h), compiled by
itself into tests/inference_driver.cpp: its p, its p < 0.05 rule and its threshold against frog_amd.volume's fwe_p, cluster_p
and tfce_p, against a count written here, and against the property the tool's header promises for threshold_p05."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from frog_amd.volume import cluster_p, fwe_p, tfce_p

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(os.path.dirname(HERE), "frog_amd", "csrc", "host")
F4, F8 = np.float32, np.float64
N_PERMS = (2, 19, 20, 21, 40, 41, 100)
SPECIAL = np.array([np.inf, -np.inf, np.nan, -0.0, 0.0], F4)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no C++ compiler")
    exe = str(tmp_path_factory.mktemp("inference") / "driver")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-I", HOST, os.path.join(HERE, "inference_driver.cpp"), "-o", exe], check=True)
    return exe


def bits(x):
    return np.ascontiguousarray(x, F4).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and (bits(a) == bits(b)).all()


def ask(driver, kind, rows, values):
    """(p float32, significant bool, threshold float64) of `values` against the null `rows` (n_perms - 1, sides)."""
    text = (lambda v: "%08x" % int(bits(v)[0])) if kind == "f" else (lambda v: str(int(v)))
    words = [kind, str(rows.shape[1]), str(len(rows))] + [text(v) for v in rows.reshape(-1)] + [str(len(values))] + [text(v) for v in values]
    r = subprocess.run([driver], input=" ".join(words), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    assert len(lines) == len(values) + 2 and lines[-1] == ""
    p = np.array([float.fromhex(l.split()[0]) for l in lines[:len(values)]], F8)
    assert (p.astype(F4) == p).all()                                            # a float32 came out
    return p.astype(F4), np.array([int(l.split()[1]) for l in lines[:len(values)]], bool), float.fromhex(lines[len(values)])


def counted(null, values, n_perms):
    """The header's formula by counting, in Python's exact arithmetic on the values as they are: p, p < 0.05, and the threshold.
    A NaN has p = 1, as the tool gives its NaN voxels."""
    exceed = [len(null) if v != v else sum(1 for x in null if x >= v) for v in values]
    p = np.array([F4(F8(1 + e) / F8(n_perms)) for e in exceed], F4)
    allowed = (n_perms - 1) // 20 - 1
    return p, np.array([20 * (1 + e) < n_perms for e in exceed], bool), np.inf if allowed < 0 else float(sorted(null)[len(null) - 1 - allowed])


def float_null(n_perms, seed):
    """Halves in [-3, 3]: ties among the null, and with the values, which are the null's own, the quarters between, and SPECIAL."""
    rng = np.random.default_rng(seed)
    null = (rng.integers(-6, 7, n_perms - 1) / 2).astype(F4)
    grid = np.arange(-14, 15, dtype=F4) / 4
    return null, np.concatenate([null, grid, SPECIAL])


def check(got, want, values, threshold_type=float):
    p, significant, threshold = got
    wp, ws, wt = want
    assert same(p, wp) and (significant == ws).all() and threshold == wt
    # what the tool's header promises: p < 0.05 exactly where the value exceeds threshold_p05
    assert (significant == np.array([threshold_type(v) > threshold for v in values], bool)).all()


@pytest.mark.parametrize("n_perms", N_PERMS)
def test_float_statistics(driver, n_perms):
    null, values = float_null(n_perms, n_perms)
    got = ask(driver, "f", null.reshape(-1, 1), values)
    check(got, counted([float(x) for x in null], [float(v) for v in values], n_perms), values)
    assert got[1].any() == (n_perms > 20)                                       # -np 20 and below can show nothing, 21 can
    row = np.concatenate([[F4(99)], null])                                      # row 0 is the design itself: no part of the null
    assert same(got[0], fwe_p(values, row))
    on = values > 0                                                             # tfce_p goes by magnitude, and gives 0 the p 1
    assert on.sum() > 14 and same(got[0][on], tfce_p(values[on], row)) and same(got[0][on], tfce_p(-values[on], row))
    assert (tfce_p(values[values == 0], row) == 1).all() and (fwe_p(values, row, fit=np.zeros(len(values), bool)) == 1).all()


@pytest.mark.parametrize("n_perms", N_PERMS)
def test_two_sided_takes_the_larger_side(driver, n_perms):
    rng = np.random.default_rng(100 + n_perms)
    max_t = (rng.integers(0, 8, n_perms) / 2).astype(F4)
    min_t = (-rng.integers(0, 10, n_perms) / 2).astype(F4)
    max_t[1], min_t[1] = 1.5, -2.5                                             # -min > max
    if n_perms > 2:
        max_t[2], min_t[2] = 3.0, -0.5                                         # and max > -min
    values = np.abs(float_null(n_perms, n_perms)[1])
    got = ask(driver, "f", np.stack([max_t[1:], -min_t[1:]], axis=1), values)
    null = np.maximum(max_t[1:], -min_t[1:])
    check(got, counted([float(x) for x in null], [float(v) for v in values], n_perms), values)
    signed = values * np.where(np.arange(len(values)) % 2, F4(-1), F4(1))      # fwe_p takes |t|
    assert same(got[0], fwe_p(signed, max_t, min_t))
    assert not same(got[0], fwe_p(values, max_t))                               # and the negative side matters


@pytest.mark.parametrize("n_perms", N_PERMS)
def test_extents(driver, n_perms):
    """uint32 extents with 0 and 2^32 - 1 among them: 2^32 - 1 and 2^32 - 2 are one float32, so a comparison that went
    through float would tie them."""
    rng = np.random.default_rng(200 + n_perms)
    top = 2 ** 32 - 1
    pool = np.array([0, 1, 5, 5, 17, top - 1, top], np.uint64)
    null = pool[rng.integers(0, len(pool), n_perms - 1)]
    null[0] = top - 1
    values = np.array([0, 1, 2, 5, 6, 17, 18, top - 2, top - 1, top], np.uint64)
    got = ask(driver, "u", null.reshape(-1, 1), values)
    check(got, counted([int(x) for x in null], [int(v) for v in values], n_perms), values, int)
    assert got[0][-1] < got[0][-2] == got[0][-3]                                # null[0] lies between the last two values
    assert same(got[0], cluster_p(values.astype(np.int64), np.concatenate([[np.uint64(7)], null]).astype(np.int64)))
    # the larger of two sides, as the tool reduces a slot pair
    other = pool[rng.integers(0, len(pool), n_perms - 1)]
    pair = ask(driver, "u", np.stack([null, other], axis=1), values)
    check(pair, counted([int(x) for x in np.maximum(null, other)], [int(v) for v in values], n_perms), values, int)
