"""The per-voxel linear model and its permutation test on the device (frog_glm, include/frog_chain.h; frog_amd.volume.GroupGLM
and group_glm; bin/GroupStats) against the restatement (glm_restate.py).  Every comparison with the restatement is == on bits,
floats through an integer view; the one exception is the logarithm of the Jacobian determinant, whose bound is derived below."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from frog_amd import _abi
from frog_amd.chain import Chain, Link, invert, read_transform
from frog_amd.volume import CoverAverage, GroupGLM, bbox_grid, fwe_p, glm_draw, glm_planes, group_glm, read_volume, write_volume

import cover_restate
import glm_restate as G
import rank_restate
from test_glm import DESIGNED_GRID, DESIGNED_PERMS, DESIGNED_SEED, designed_case, designed_condition
from test_gpu_cover import ALL_TYPES, GRID, SRC_S, SRC_SHAPE, OFFSETS, affine_links, masks, same
from test_gpu_cover import device as cover_device
from test_gpu_rank import NONLINEAR_GRID, special_images

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.path.join(ROOT, "bin")
F4, F8 = np.float32, np.float64
LDS_MAX = 48                                                # the largest n_images whose values stay in LDS (k_glm.hip.h)
SHAPE = GRID[0][::-1]
V = int(np.prod(SHAPE))


def design(n, p, seed=3):
    """An intercept, an alternating group, a centred index, then noise: the first p of them."""
    rng = np.random.default_rng(seed)
    cols = [np.ones(n), (np.arange(n) % 2).astype(F8), np.arange(n) - (n - 1) / 2.0] + [rng.normal(size=n) for _ in range(5)]
    return np.stack(cols[:p], axis=1)


def same_all(got, want):
    return len(got) == len(want) and all(same(g, w) for g, w in zip(got, want))


# ---- 1. planes ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,mode", [(d, 1) for d in ALL_TYPES] + [("int16", 0), ("float32", 0)])
def test_planes_equal_the_restatement(dtype, mode):
    images = special_images(dtype)                          # the float sources hold +-inf and NaN
    m_u8, m_i16 = masks()
    images = [(l, v, o, s, (None, m_u8, m_i16, None, m_u8)[k]) for k, (l, v, o, s, _) in enumerate(images)]
    want = G.collect(images, GRID, mode, 3.0)
    acc = GroupGLM(GRID, design(5, 2))
    with pytest.raises(_abi.FrogError) as e:
        acc.plane(0)                                        # not added yet
    assert e.value.code == _abi.FROG_E_INVALID
    for links, vol, o, s, mask in images:
        acc.add((vol, o, s), Chain(links), mask, mode, 3.0)
    got = np.stack([acc.plane(i) for i in range(5)])
    assert same(got, want)
    taking = ~np.isnan(want)
    assert taking.any() and not taking.all() and np.isfinite(got[taking]).all()
    assert (got.view(np.uint32)[~taking] == 0x7FC00000).all()
    # the entries take part where frog_rank's do, minus the infinities
    keys = rank_restate.collect(images, GRID, mode, 3.0)
    assert (taking <= (keys != rank_restate.SENTINEL)).all()
    if np.dtype(dtype).kind == "f" and mode == 1:
        assert (taking < (keys != rank_restate.SENTINEL)).any()
    with pytest.raises(_abi.FrogError) as e:
        acc.add((images[0][1], images[0][2], images[0][3]), Chain(images[0][0]))        # the sixth of five
    assert e.value.code == _abi.FROG_E_INVALID
    acc.close()


# ---- 2. Jacobian -------------------------------------------------------------------------------------------------------------

def ordered(x):
    return rank_restate.keys_of(x).astype(np.int64)


def test_jacobian_planes():
    from test_gpu_chain import random_chain
    rng = np.random.default_rng(83)
    chain = Chain(random_chain(rng, 2, 1.0))
    dims, origin, spacing = NONLINEAR_GRID
    det64 = chain.sample(origin, spacing, dims, displacement=False, dtype=np.float64)[1]
    assert det64.min() > 0 and det64.std() > 0.01
    acc = GroupGLM(NONLINEAR_GRID, np.ones((3, 1)))
    acc.add_jacobian(chain, log=False)
    acc.add_jacobian(chain, log=True)
    assert same(acc.plane(0), det64.astype(F4))
    # HIP's device math table gives the f64 log 1 ulp; np.log is within 1 ulp too, so the two f64 values lie within 2 f64 ulps of
    # each other and their f32 casts are equal or neighbours: one f32 ulp
    got, want = acc.plane(1), np.log(det64).astype(F4)
    assert np.abs(ordered(got) - ordered(want)).max() <= 1
    # a window of its own: the same planes, cut
    part = GroupGLM(NONLINEAR_GRID, np.ones((3, 1)), window=(4, 5))
    part.add_jacobian(chain, log=False)
    assert same(part.plane(0), det64.astype(F4)[4:9])
    part.close()
    # a reflecting affine link folds every voxel: the logarithm leaves all of them out
    mirror = Chain([Link.linear(np.diag([-1.0, 1.0, 1.0, 1.0]))])
    acc.add_jacobian(mirror, log=True)
    assert (acc.plane(2).view(np.uint32) == 0x7FC00000).all()
    _, _, _, count = acc.finish([[1.0]])
    assert (count == 2).all()
    acc.close()
    acc = GroupGLM(NONLINEAR_GRID, np.ones((2, 1)))
    acc.add_jacobian(mirror, log=False)
    assert (acc.plane(0) == -1).all()
    with pytest.raises(_abi.FrogError) as e:
        acc.add_jacobian(None)
    assert e.value.code == _abi.FROG_E_INVALID
    with pytest.raises(_abi.FrogError) as e:
        acc.add_jacobian(mirror, mask=(np.ones((3, 3, 3), F4), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)))       # a float mask
    assert e.value.code == _abi.FROG_E_INVALID
    with pytest.raises(_abi.FrogError) as e:
        acc.add_jacobian(mirror, support=((3, 3, 3), (0.0, 0.0, 0.0), (1.0, 0.0, 1.0)))                 # a spacing of 0
    assert e.value.code == _abi.FROG_E_INVALID
    acc.close()


def test_jacobian_support_and_mask_count_as_cover_average():
    m_u8, m_i16 = masks()
    rng = np.random.default_rng(7)
    images = [(affine_links(k), rng.integers(1, 100, SRC_SHAPE).astype(np.int16), (0.0, 0.0, 0.0), SRC_S, (m_u8, None, m_i16, m_u8, None)[k])
              for k in range(5)]
    want = cover_device(images, GRID)[2]
    assert sorted(np.unique(want)) == [0, 1, 2, 3, 4, 5]
    acc = GroupGLM(GRID, np.ones((5, 1)))
    for links, vol, o, s, mask in images:
        acc.add_jacobian(Chain(links), (vol.shape[::-1], o, s), mask, log=True)
    assert same(acc.finish([[1.0]])[3], want)
    acc.close()


# ---- 3. fit ------------------------------------------------------------------------------------------------------------------

PLANTED = dict(nobody=0, one_group=300, k_is_p=1000, k_is_p1=2000, constant=3000, exact=4198)


def fit_group(p, n=12, seed=41):
    """n float volumes on GRID with on-grid masks (no chain): a quarter of the entries dropped at random, and the planted
    voxels.  Returns (volumes, masks uint8, design)."""
    rng = np.random.default_rng(seed + p)
    X = design(n, p)
    vols = rng.normal(0, 1, (n, V)).astype(F4)
    vols[:, 500:900] += F4(2) * X[:, min(1, p - 1), None].astype(F4)
    on = rng.random((n, V)) >= 0.25
    on[:, PLANTED["nobody"]] = False
    on[:, PLANTED["one_group"]] = (np.arange(n) % 2 == 0)
    on[:, PLANTED["k_is_p"]] = np.arange(n) < p
    on[:, PLANTED["k_is_p1"]] = np.arange(n) < p + 1
    on[:, PLANTED["constant"]] = True
    vols[:, PLANTED["constant"]] = 2.5
    on[:, PLANTED["exact"]] = True
    vols[:, PLANTED["exact"]] = (X[:, :min(p, 2)] @ np.array([3.0, -2.0])[:min(p, 2)]).astype(F4)      # exact in f32
    return vols.reshape((n,) + SHAPE), on.astype(np.uint8).reshape((n,) + SHAPE), X


def device_group(vols, on, X, window=None):
    acc = GroupGLM(GRID, X, window)
    for v, m in zip(vols, on):
        acc.add(v, None, m)
    return acc


def contrasts_of(p, n_c):
    if n_c == 1:
        return np.eye(p)[p - 1:p]
    rng = np.random.default_rng(100 + p)
    c = rng.integers(-2, 3, (8, p)).astype(F8)
    c[0], c[1] = np.eye(p)[0], 0.0                           # the intercept alone; a zero contrast, whose t is 0 / 0
    return c


@pytest.mark.parametrize("n_c", [1, 8])
@pytest.mark.parametrize("p", [1, 2, 3, 8])
def test_fit_equals_the_restatement(p, n_c):
    vols, on, X = fit_group(p)
    planes = np.where(on != 0, vols, G.NAN)
    cons = contrasts_of(p, n_c)
    region = np.ones(SHAPE, np.uint8)
    region[3:5, 2:9, 4:11] = 0
    acc = device_group(vols, on, X)
    for min_count, sigma_floor, reg, fill in ((1, 0.0, None, 0.0), (7, 1e-6, region, -9.0)):
        want = G.finish(planes, X, cons, min_count, sigma_floor, reg, fill)
        beta, sigma, t, count, fit = (w.reshape(w.shape[:-3] + (-1,)) for w in want)
        at = PLANTED
        assert count[at["nobody"]] == 0 and not fit[at["nobody"]]
        assert count[at["k_is_p"]] == p and not fit[at["k_is_p"]]
        assert count[at["k_is_p1"]] == p + 1 and fit[at["k_is_p1"]] == (min_count <= p + 1)
        assert count[at["one_group"]] == 6 and fit[at["one_group"]] == (p == 1 and min_count <= 6)     # a column of zeros has no pivot
        assert count[at["constant"]] == 12 and fit[at["constant"]] and fit[at["exact"]]
        assert same(t[:, ~fit], np.full((n_c, int((~fit).sum())), F4(fill))) and (sigma[~fit] == F4(fill)).all()
        if p == 1:                                          # a constant value is an exact fit of the intercept: sd is 0
            assert sigma[at["constant"]] == 0 and (t[:, at["constant"]].view(np.uint32) == 0x7FC00000).all()
        if sigma_floor:                                     # the planted exact fit leaves rounding noise at most
            assert sigma[at["exact"]] <= sigma_floor and (t[:, at["exact"]].view(np.uint32) == 0x7FC00000).all()
        if n_c == 8:
            assert (t[1, fit].view(np.uint32) == 0x7FC00000).all()
        finite = fit & ~np.isnan(t[0])
        assert finite.sum() > V // 3 and np.isfinite(t[:, fit][~np.isnan(t[:, fit])]).all()
        if reg is not None:
            assert not fit.reshape(SHAPE)[3:5, 2:9, 4:11].any() and (count.reshape(SHAPE)[3:5, 2:9, 4:11] > 0).any()
        got = acc.finish(cons, min_count, sigma_floor, reg, fill)
        assert same_all(got, want[:4]), (p, n_c, min_count)
    # any single output has the bits it has beside the others; no output at all is refused
    lib, con = acc._lib, cons.ctypes.data_as(_abi.c_double_p)
    alone = np.empty((n_c,) + SHAPE, F4)
    assert lib.frog_glm_finish(acc._h, n_c, con, 7, 1e-6, region.ctypes.data_as(C.POINTER(C.c_uint8)), -9.0, None, None,
                               alone.ctypes.data_as(_abi.c_float_p), None) == _abi.FROG_OK
    assert same(alone, want[2])
    assert lib.frog_glm_finish(acc._h, n_c, con, 1, 0.0, None, 0.0, None, None, None, None) == _abi.FROG_E_INVALID
    acc.close()


def test_finish_and_permute_refuse_before_the_device_is_touched():
    vols, on, X = fit_group(2)
    acc = GroupGLM(GRID, X)
    lib = acc._lib
    f = np.empty(16 * V, F4).ctypes.data_as(_abi.c_float_p)
    con = (C.c_double * 18)(*([0.0, 1.0] * 9))
    perm, sign = glm_draw(12, 2, 1, True, True)
    pp, sp = perm.ctypes.data_as(_abi.c_u32_p), sign.ctypes.data_as(C.POINTER(C.c_int8))

    def finish(n_c=1, c=con, mc=1, sf=0.0):
        return lib.frog_glm_finish(acc._h, n_c, c, mc, sf, None, 0.0, f, f, f, None)

    def permute(n_c=1, c=con, mc=1, sf=0.0, cols=2, k=2, pm=pp, sg=sp, hi=f, lo=f):
        return lib.frog_glm_permute(acc._h, n_c, c, mc, sf, None, cols, k, pm, sg, hi, lo)

    for v, m in zip(vols[:11], on[:11]):
        acc.add(v, None, m)
    assert finish() == _abi.FROG_E_INVALID and permute() == _abi.FROG_E_INVALID                  # eleven adds of twelve
    acc.add(vols[11], None, on[11])
    assert finish() == _abi.FROG_OK and permute() == _abi.FROG_OK
    for bad in (dict(mc=0), dict(n_c=9), dict(c=None), dict(sf=-1.0), dict(sf=float("nan"))):
        assert finish(**bad) == _abi.FROG_E_INVALID and permute(**bad) == _abi.FROG_E_INVALID, bad
    con[1] = float("inf")
    assert finish() == _abi.FROG_E_INVALID and permute() == _abi.FROG_E_INVALID
    con[1] = 1.0
    for bad in (dict(n_c=0), dict(k=0), dict(pm=None), dict(cols=0), dict(cols=4), dict(cols=7), dict(hi=None, lo=None)):
        assert permute(**bad) == _abi.FROG_E_INVALID, bad
    assert permute(sg=None) == _abi.FROG_OK and permute(hi=None) == _abi.FROG_OK
    perm[1, 3] = 12
    assert permute() == _abi.FROG_E_INVALID
    perm[1, 3] = 3
    for value in (0, 2, -2):
        sign[1, 5] = value
        assert permute() == _abi.FROG_E_INVALID, value
    acc.close()


# ---- 4. image counts ---------------------------------------------------------------------------------------------------------

SMALL = ((5, 4, 3), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


@pytest.mark.parametrize("n", [LDS_MAX, LDS_MAX + 1, 200])
def test_image_counts(n):
    rng = np.random.default_rng(n)
    X = design(n, 2)
    vols = rng.normal(0, 1, (n, 3, 4, 5)).astype(F4) + X[:, 1, None, None, None].astype(F4)
    on = (rng.random((n, 3, 4, 5)) >= 0.2).astype(np.uint8)
    on[:, 0, 0, 0] = 0
    planes = np.where(on != 0, vols, G.NAN)
    acc = GroupGLM(SMALL, X)
    for v, m in zip(vols, on):
        acc.add(v, None, m)
    cons = [[0.0, 1.0], [1.0, -1.0]]
    want = G.finish(planes, X, cons, 3, 0.0, None, -1.0)
    assert want[4].sum() == 59 and want[3].max() > n * 0.6
    assert same_all(acc.finish(cons, 3, 0.0, None, -1.0), want[:4])
    perm, sign = glm_draw(n, 3, n, True, True)
    assert same_all(acc.permute(cons, perm, sign, [1], 3), G.permute(planes, X, cons, perm, sign, 2, 3))
    acc.close()


# ---- 5. windows, 6. permutations ---------------------------------------------------------------------------------------------

def chained_group(n=12):
    """n float sources on test_gpu_cover's source geometries, through its sheared affine chains, two with masks of another
    geometry."""
    rng = np.random.default_rng(19)
    m_u8, m_i16 = masks()
    vols = [(rng.normal(0, 1, SRC_SHAPE).astype(F4) + F4(k % 2), tuple(0.25 * (k // 5) for _ in range(3)), SRC_S) for k in range(n)]
    links = [affine_links(k % len(OFFSETS)) for k in range(n)]
    mks = [(m_u8, m_i16, None)[k % 3] for k in range(n)]
    return vols, links, mks


def window_outputs():
    """The chained group through group_glm whole and in windows of 1, 5 and 7 planes, with 6 permutations and sign flips."""
    vols, links, mks = chained_group()
    chains = [Chain(l) for l in links]
    out = {}
    for planes in (13, 1, 5, 7):
        r = group_glm(design(12, 3), [[0, 1, 0], [0, 0, 1]], vols, chains, mks, GRID, "images", min_count=5, fill=-3.0, n_perms=6, seed=8, flip=True,
                      two_sided=True, max_planes=planes)
        for k, v in r.items():
            out[f"{k}_{planes}"] = v
    return out


def test_windows_and_launch_chunks(tmp_path):
    vols, links, mks = chained_group()
    X, cons = design(12, 3), np.array([[0.0, 1, 0], [0, 0, 1]])
    chained = [(Chain(l), v, o, s, m) for l, (v, o, s), m in zip(links, vols, mks)]
    planes = G.collect(chained, GRID, reslicer=lambda c, *a: c.reslice(*a))
    want = G.finish(planes, X, cons, 5, 0.0, None, -3.0)
    perm, sign = G.draw(12, 6, 8, True, True)
    hi, lo = G.permute(planes, X, cons, perm, sign, 6, 5)
    assert want[4].any() and not want[4].all() and len(np.unique(want[3])) > 4
    assert glm_planes(GRID, 12) == 13
    plain = window_outputs()
    for w in (13, 1, 5, 7):
        for name, value in zip(("beta", "sigma", "t", "count", "fit"), want):
            assert same(plain[f"{name}_{w}"], value), (name, w)
        assert same(plain[f"max_t_{w}"], hi) and same(plain[f"min_t_{w}"], lo), w
        assert same(plain[f"p_{w}"], np.stack([fwe_p(want[2][j], hi[:, j], lo[:, j], want[4]) for j in range(2)])), w
    # small launch chunks (FROG_CHAIN_LAUNCH_MAX is read once per process: a child)
    path = str(tmp_path / "chunks.npz")
    code = "import sys; sys.path[:0] = [%r, %r]; import numpy as np, test_gpu_glm as t; np.savez(%r, **t.window_outputs())" % (ROOT, HERE, path)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, FROG_CHAIN_LAUNCH_MAX="512"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    chunked = dict(np.load(path))
    assert sorted(chunked) == sorted(plain) and len(plain) == 32
    for k, v in plain.items():
        assert v.dtype == chunked[k].dtype and v.tobytes() == chunked[k].tobytes(), k


@pytest.mark.parametrize("columns", [[1], [0, 1, 2]])
def test_permutations_equal_the_restatement(columns):
    vols, on, X = fit_group(3)
    planes = np.where(on != 0, vols, G.NAN)
    cons = np.array([[0.0, 1, 0], [0, 0, 1], [1, 0, 0]])
    perm, sign = glm_draw(12, 16, 77, True, True)
    assert same_all((perm, sign), G.draw(12, 16, 77, True, True))
    bits = sum(1 << j for j in columns)
    want = G.permute(planes, X, cons, perm, sign, bits, 5)
    assert np.isfinite(want[0]).all() and (want[0] > want[1]).all() and len(np.unique(want[0][:, 0])) == 16
    acc = device_group(vols, on, X)
    got = acc.permute(cons, perm, sign, columns, 5)
    assert same_all(got, want)
    assert same_all(acc.permute(cons, perm, sign, bits, 5), got)                    # a second run: the same bits
    # row 0 is the design itself: the extrema of finish's t over the fit voxels
    _, _, t, _, fit = G.finish(planes, X, cons, 5)
    assert same_all(acc.finish(cons, 5)[2:3], (t,))
    for c in range(3):
        values = t[c][fit & ~np.isnan(t[c])]
        assert got[0][0, c] == np.nanmax(values) and got[1][0, c] == np.nanmin(values)
    # two calls of 8 are one call of 16
    a, b = acc.permute(cons, perm[:8], sign[:8], columns, 5), acc.permute(cons, perm[8:], sign[8:], columns, 5)
    assert same(np.concatenate([a[0], b[0]]), got[0]) and same(np.concatenate([a[1], b[1]]), got[1])
    # without signs: all + 1
    assert same_all(acc.permute(cons, perm, None, columns, 5), G.permute(planes, X, cons, perm, None, bits, 5))
    acc.close()
    # the extrema of windows combine to the whole grid's
    hi, lo = np.full((16, 3), -np.inf, F4), np.full((16, 3), np.inf, F4)
    for first, n in ((0, 4), (4, 1), (5, 8)):
        part = device_group(vols, on, X, window=(first, n))      # on-grid sources stay grid-sized
        h, l = part.permute(cons, perm, sign, columns, 5)
        part.close()
        hi, lo = np.where(ordered(h) > ordered(hi), h, hi), np.where(ordered(l) < ordered(lo), l, lo)
    assert same(hi, got[0]) and same(lo, got[1])


def test_designed_case_on_the_device():
    vols, on, X, con, block = designed_case()
    planes = np.where(on != 0, vols, G.NAN)
    r = group_glm(X, con, list(vols), None, list(on), DESIGNED_GRID, "images", n_perms=DESIGNED_PERMS, seed=DESIGNED_SEED)
    want = G.finish(planes, X, con)
    perm, _ = G.draw(len(X), DESIGNED_PERMS, DESIGNED_SEED)
    hi, lo = G.permute(planes, X, con, perm, None, 2)
    assert same_all([r[k] for k in ("beta", "sigma", "t", "count", "fit")], want)
    assert same(r["max_t"], hi) and same(r["min_t"], lo)
    assert same(r["p"][0], fwe_p(want[2][0], hi[:, 0], fit=want[4]))
    designed_condition(r["p"][0], r["t"][0], r["fit"], block)


# ---- 7. the tool -------------------------------------------------------------------------------------------------------------

def run(args, cwd, timeout=300):
    return subprocess.run(args, cwd=cwd, capture_output=True, text=True, timeout=timeout)


def test_group_stats_end_to_end(tmp_path):
    from test_chain import smooth_chain
    from test_gpu_chain import _write_chain
    d = tmp_path
    rng = np.random.default_rng(61)
    n = 8
    (d / "bbox.json").write_text(json.dumps({"bbox": [[0.0, 0.0, 0.0], [60.0, 52.0, 44.0]]}))
    (d / "transforms").mkdir()
    names, mask_names = [], []
    z, y, x = np.meshgrid(np.arange(14), np.arange(16), np.arange(18), indexing="ij")
    for i in range(n):
        _write_chain(d / "transforms" / f"{i}.json", smooth_chain(seed=70 + i, amplitude=1.5))
        v = (100 + 60 * np.sin(x / (3.0 + i % 3)) * np.cos(y / 4.0) + 5 * z + rng.normal(0, 2, x.shape) + 10 * (i % 2)).astype(("int16", "float32")[i % 2])
        names.append(f"v{i}.nii.gz")
        write_volume(d / names[-1], v, (2.0 + 2.0 * (i % 4), 1.0 + 1.5 * (i % 3), 1.0 * (i % 2)), (3.5, 3.5, 3.5))
        m = (rng.integers(0, 5, (10, 10, 10)) > 0).astype(("uint8", "int16")[i % 2])
        mask_names.append(f"m{i}.nii.gz")
        write_volume(d / mask_names[-1], m, (3.0 + 1.0 * i, 2.0, 1.0), (6.0, 6.0, 6.0))
    (d / "volumes.txt").write_text("\n".join(names) + "\n")
    (d / "masks.txt").write_text("\n".join(mask_names) + "\n")
    X = np.stack([np.ones(n), np.arange(n) % 2, np.array([31, 45, 52, 38, 60, 27, 49, 55.0])], axis=1)
    (d / "design.csv").write_text("intercept,group,age\n" + "\n".join(",".join(repr(float(v)) for v in row) for row in X) + "\n")
    (d / "contrasts.csv").write_text("0 1 0\n0,0,-1\n")
    spacing = "4"
    grid = bbox_grid(d / "bbox.json", float(spacing))
    assert grid[0][2] == 11
    region = np.ones(grid[0][::-1], np.uint8)
    region[:, :2] = 0
    write_volume(d / "region.nii.gz", region, grid[1], grid[2])
    tool = [os.path.join(BIN, "GroupStats"), "bbox.json", spacing, "design.csv"]
    common = ["-vl", "volumes.txt", "-ml", "masks.txt", "-m", "region.nii.gz", "-mc", "5", "-f", "-5", "-np", "20", "-ps", "9", "-two", "1"]
    r = run(tool + ["-o", "whole"] + common, d)
    assert r.returncode == 0 and "stats : 1 slab of 11 planes" in r.stdout, r.stdout + r.stderr
    r = run(tool + ["-o", "slabs", "-rp", "3"] + common, d)
    assert r.returncode == 0 and "stats : 4 slabs of 3 planes" in r.stdout, r.stdout + r.stderr
    vols = [read_volume(d / v) for v in names]
    mask_vols = [read_volume(d / m) for m in mask_names]
    chains = [Chain(invert(read_transform(d / "transforms" / f"{i}.json"))) for i in range(n)]
    supports = [(v.shape[::-1], o, s) for v, o, s in vols]
    cons = [[0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]                # the default contrasts: one per column that is not constant
    res = group_glm(X, cons, None, chains, mask_vols, grid, "logjacobian", supports, min_count=5, region=region, fill=-5.0, n_perms=20, seed=9,
                    two_sided=True)
    assert res["fit"].any() and not res["fit"][:, :2].any() and (res["count"] < 8).any() and len(np.unique(res["p"])) > 2
    files = {"sigma.nii.gz": res["sigma"], "count.nii.gz": res["count"]}
    for j in range(3):
        files[f"beta_{j}.nii.gz"] = res["beta"][j]
    for c in range(2):
        files[f"t_{c}.nii.gz"], files[f"fwe_p_{c}.nii.gz"] = res["t"][c], res["p"][c]
    for name, w in files.items():
        got, o, s = read_volume(d / "whole" / name)
        assert same(got, w) and o == grid[1] and s == grid[2], name
    for name in list(files) + ["maxt.csv", "glm.csv"]:
        assert (d / "slabs" / name).read_bytes() == (d / "whole" / name).read_bytes(), name
    rows = np.loadtxt(d / "whole" / "maxt.csv", delimiter=",", skiprows=1).reshape(20, 2, 4)
    assert same(rows[:, :, 2].astype(F4), res["max_t"]) and same(rows[:, :, 3].astype(F4), res["min_t"])
    # fwe_p follows the stated formula from maxt.csv
    for c in range(2):
        null = np.maximum(rows[1:, c, 2], -rows[1:, c, 3]).astype(F4)
        t, p = read_volume(d / "whole" / f"t_{c}.nii.gz")[0], read_volume(d / "whole" / f"fwe_p_{c}.nii.gz")[0]
        for v in np.flatnonzero(res["fit"].reshape(-1))[::53]:
            tv = t.reshape(-1)[v]
            assert p.reshape(-1)[v] == (1 if np.isnan(tv) else F4((1 + int((null >= abs(tv)).sum())) / F8(20)))
        assert (p[~res["fit"]] == 1).all()
    table = (d / "whole" / "glm.csv").read_text().splitlines()
    assert table[0] == "contrast,fit_voxels,peak_t,peak_x,peak_y,peak_z,threshold_p05,voxels_p05" and len(table) == 3
    for c in range(2):
        f = table[1 + c].split(",")
        tc = res["t"][c]
        counted = res["fit"] & ~np.isnan(tc)
        assert int(f[0]) == c and int(f[1]) == counted.sum() and float(f[2]) == tc[int(f[5]), int(f[4]), int(f[3])]
        assert abs(float(f[2])) == np.abs(tc[counted]).max() and f[6] == "inf" and int(f[7]) == 0       # 20 permutations: p >= 0.05
    # the explicit contrasts; intensities instead of determinants
    r = run(tool + ["-o", "images", "-v", "images", "-c", "contrasts.csv", "-vl", "volumes.txt", "-mc", "5", "-np", "4", "-pc", "1,2", "-pf", "1"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    res = group_glm(X, [[0, 1, 0], [0, 0, -1]], vols, chains, None, grid, "images", min_count=5, n_perms=4, columns=[1, 2], flip=True)
    for name, w in (("t_0.nii.gz", res["t"][0]), ("t_1.nii.gz", res["t"][1]), ("fwe_p_1.nii.gz", res["p"][1]), ("beta_2.nii.gz", res["beta"][2])):
        assert same(read_volume(d / "images" / name)[0], w), name
    # refused before anything is written
    (d / "short.csv").write_text("1,0\n1,1\n")
    (d / "wide.csv").write_text("0 1\n")
    for k, extra in enumerate((["-np", "1"], ["-ps", "3"], ["-v", "images"], ["-v", "volume"], ["-c", "wide.csv"], ["-pc", "3", "-np", "5"],
                               ["-td", "nowhere"], ["-vl", "masks.txt", "-m", "m0.nii.gz"], ["-rp", "0"], ["-mc", "0"])):
        r = run(tool + ["-o", f"bad{k}"] + extra, d)
        assert r.returncode != 0 and not (d / f"bad{k}").exists(), extra
    r = run([tool[0], "bbox.json", spacing, "short.csv", "-o", "bad_design"], d)
    assert r.returncode != 0 and not (d / "bad_design").exists()
