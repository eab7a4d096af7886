"""The principal modes of a group on the device (frog_modes, include/frog_chain.h; frog_amd.volume.ModeImages, group_modes;
bin/GroupModes) against the restatement (modes_restate.py).  Every comparison is == on bits unless it says otherwise.

The designed case (test_modes.py): 12 images on a 13 x 11 x 9 grid, 3 components, field_i = mean + sum_k B_ik sd_k psi_k
with sd = 4, 2, 1 mm, planted here as FROG_T_FIELD links on the sampling grid, under test_modes' bars: modes within 2^-21 x the
largest stored magnitude, eigenvalues and scores within 2^-21 relative, the fourth rms below 2^-21 x the first."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

from frog_amd import _abi
from frog_amd.chain import Chain, Link, invert, read_nifti_lattice, read_transform
from frog_amd.volume import GroupGLM, ModeImages, bbox_grid, drop_linear, group_modes, modes_planes, read_volume, write_group_modes

import modes_restate as R
from test_gpu_clusters import N_TOOL, SPACING, tool_dir      # noqa: F401  (the fixture: the small registered group of the tool tests)
from test_gpu_glm import chained_group
from test_gpu_cover import GRID
from test_gpu_rank import NONLINEAR_GRID
from test_modes import check_designed

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BIN = os.path.join(os.path.dirname(HERE), "bin")
F4, F8 = np.float32, np.float64
TILE = 32                                                   # MODES_TILE of k_modes.hip.h: the images of a tile


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def unit_grid(dims):
    return (dims, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


def field_chain(grid, values):
    dims, origin, spacing = grid
    return Chain([Link.field(dims, origin, spacing, np.ascontiguousarray(values, F4).reshape(-1, 3))])


def filled(grid, images, components, window=None, masks=None):
    """A ModeImages with `images` added: grid-sized float32 volumes without a chain (1 component), or fields planted through
    a FROG_T_FIELD link on the grid itself (3 components)."""
    acc = ModeImages(grid, len(images), components, window)
    for k, v in enumerate(images):
        mask = None if masks is None else masks[k]
        if components == 1:
            acc.add(v, None, mask)
        else:
            acc.add_displacement(field_chain(grid, v), None, None if mask is None else (mask, grid[1], grid[2]))
    return acc


def planes_of(acc):
    return np.stack([acc.plane(i) for i in range(acc.n_images)])


# ---- 4. planes -----------------------------------------------------------------------------------------------------------------

def test_displacement_planes_equal_the_sampled_field():
    from test_gpu_chain import random_chain
    chain = Chain(random_chain(np.random.default_rng(83), 2, 1.0))                 # a linear link and two lattices
    dims, origin, spacing = NONLINEAR_GRID
    want = chain.sample(origin, spacing, dims, determinant=False)[0]
    assert want.dtype == F4 and want.std() > 0.5
    acc = ModeImages(NONLINEAR_GRID, 2, 3)
    with pytest.raises(_abi.FrogError) as e:
        acc.plane(0)                                        # not added yet
    assert e.value.code == _abi.FROG_E_INVALID
    acc.add_displacement(chain)
    # a support the chain leaves, and a mask: as GroupGLM.add_jacobian counts them
    support = ((10, 11, 12), (8.0, 10.0, 6.0), (4.0, 4.0, 4.0))
    mask = ((np.random.default_rng(5).integers(0, 3, (9, 9, 9)) > 0).astype(np.uint8), (10.0, 10.0, 6.0), (6.0, 6.0, 6.0))
    acc.add_displacement(chain, support, mask)
    assert same(acc.plane(0), want)
    glm = GroupGLM(NONLINEAR_GRID, np.ones((2, 1)))
    glm.add_jacobian(chain, support, mask, log=False)
    valid = ~np.isnan(glm.plane(0))
    got = acc.plane(1)
    assert valid.any() and not valid.all()
    assert same(got[valid], want[valid]) and (got[~valid].view(np.uint32) == R.NAN_BITS).all()
    acc.close()
    glm.close()
    part = ModeImages(NONLINEAR_GRID, 2, 3, window=(4, 5))
    part.add_displacement(chain)
    assert same(part.plane(0), want[4:9])
    part.close()


def test_scalar_planes_equal_group_glm():
    from test_gpu_chain import random_chain
    vols, links, mks = chained_group(5)
    chain = Chain(random_chain(np.random.default_rng(83), 2, 1.0))
    for window in (None, (3, 6)):
        acc, glm = ModeImages(GRID, 5, 1, window), GroupGLM(GRID, np.ones((5, 1)), window)
        for v, l, m in zip(vols, links, mks):
            acc.add(v, Chain(l), m)
            glm.add(v, Chain(l), m)
        taking = ~np.isnan(glm.plane(1))
        assert taking.any() and not taking.all()
        assert all(same(acc.plane(i), glm.plane(i)) for i in range(5))
        acc.close()
        glm.close()
    acc, glm = ModeImages(NONLINEAR_GRID, 2, 1), GroupGLM(NONLINEAR_GRID, np.ones((2, 1)))
    for log in (False, True):
        acc.add_jacobian(chain, log=log)
        glm.add_jacobian(chain, log=log)
    assert same(acc.plane(0), glm.plane(0)) and same(acc.plane(1), glm.plane(1)) and acc.plane(0).std() > 0.01
    acc.close()
    glm.close()


def test_planted_fields_come_back():
    """A FROG_T_FIELD link on the sampling grid: at its own nodes the chain's displacement is the planted value, exactly where
    node + value is exact in float64 (dyadic values here)."""
    grid = ((7, 5, 4), (-3.0, 2.0, 1.0), (2.0, 1.5, 0.5))
    rng = np.random.default_rng(2)
    fields = (rng.integers(-4096, 4096, (3, 4, 5, 7, 3)) / 64.0).astype(F4)
    fields[1, 0, 0, 0] = [0.0, -0.0, 3e38]
    acc = filled(grid, fields, 3)
    got = planes_of(acc)
    fields[1, 0, 0, 0, 1] = 0.0                             # node + (-0.0) - node is +0.0
    assert same(got, fields)
    acc.close()


# ---- 5. gram, 6. projection ----------------------------------------------------------------------------------------------------

def special_volumes(n, dims, seed):
    """n float32 volumes with +-0.0, denormals, +-3e38, and entries that take no part (+-inf, NaN) in image 1."""
    rng = np.random.default_rng(seed)
    shape = dims[::-1]
    v = rng.normal(0, 2, (n,) + shape).astype(F4)
    flat = v.reshape(n, -1)
    count = flat.shape[1]
    specials = np.array([0.0, -0.0, 1e-45, -1e-40, 3e38, -3e38], F4)
    for i in range(n):
        at = rng.permutation(count)[:6]
        flat[i, at] = specials[rng.permutation(6)]
    flat[1 % n, rng.permutation(count)[:3]] = np.array([np.inf, -np.inf, np.nan], F4)
    return v


def region_of(dims, seed):
    rng = np.random.default_rng(seed)
    region = (rng.random(dims[::-1]) < 0.85).astype(np.uint8)
    region[dims[2] // 2] = 0                                # a plane wholly outside the support
    return region


def gram_case(n, components, dims, seed=1):
    """(acc, planes as stored, region)."""
    grid = unit_grid(dims)
    region = region_of(dims, seed + 1)
    if components == 1:
        acc = filled(grid, special_volumes(n, dims, seed), 1)
    else:
        rng = np.random.default_rng(seed)
        fields = rng.normal(0, 2, (n,) + dims[::-1] + (3,)).astype(F4)
        fields[0, 0, 0, 0] = [3e38, -3e38, 0.0]
        holes = (rng.random(dims[::-1]) < 0.9).astype(np.uint8)
        acc = filled(grid, fields, 3, masks=[holes if k == 1 else None for k in range(n)])
    return acc, planes_of(acc), region


COUNTS = (2, 3, TILE - 1, TILE, TILE + 1)
# (5, 3, 2): a plane holds fewer values than a chunk; (32, 32, 2): an exact multiple of it (1024 and 3072 values); (37, 21, 13):
# three and seven chunks with a short last one
CASES = [(n, c, (5, 3, 2)) for n in COUNTS for c in (1, 3)] + [(n, c, d) for n in (3, TILE + 1) for c in (1, 3) for d in ((37, 21, 13), (32, 32, 2))]


@pytest.mark.parametrize("n,components,dims", CASES)
def test_gram_and_projection_equal_the_restatement(n, components, dims):
    acc, planes, region = gram_case(n, components, dims)
    taking = planes.view(np.uint32) != R.NAN_BITS
    assert np.isfinite(planes[taking]).all() and not taking.all()
    start = np.random.default_rng(9).normal(size=n * (n + 1) // 2)
    for reg, g0, s0 in ((region, None, 0), (None, start, 17)):
        want, want_support = R.gram(planes, reg, g0, s0)
        got, support = acc.gram(reg, g0, s0)
        assert support == want_support and 0 < support - s0 < int(np.prod(dims))
        assert same(got, want) and np.isfinite(got).all()
    # an empty support leaves both as they were passed
    got, support = acc.gram(np.zeros_like(region), start, 17)
    assert same(got, start) and support == 17
    rng = np.random.default_rng(n)
    for k in sorted({1, min(3, n), n}):
        w = rng.normal(size=(k, n))
        w[0, 0], w[-1, -1] = 0.0, -0.0
        got = acc.project(w, region, -7.5)
        want = R.project(planes, w, region, -7.5)
        assert same(got[0], want[0]) and same(got[1], want[1]), k
        assert (got[0][region == 0] == -7.5).all() and (got[1][:, dims[2] // 2] == -7.5).all()
    acc.close()


# ---- 7. windows ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("components", [1, 3])
def test_windows_chained_in_ascending_order_equal_the_whole_grid(components):
    n, dims = 5, (37, 21, 7)
    grid = unit_grid(dims)
    region = region_of(dims, 4)
    rng = np.random.default_rng(6)
    images = special_volumes(n, dims, 3) if components == 1 else rng.normal(0, 2, (n,) + dims[::-1] + (3,)).astype(F4)
    w = rng.normal(size=(3, n))
    whole = filled(grid, images, components)
    gram, support = whole.gram(region)
    mean, modes = whole.project(w, region, 1.25)
    again = whole.gram(region)
    assert same(again[0], gram) and again[1] == support and all(same(a, b) for a, b in zip(whole.project(w, region, 1.25), (mean, modes)))
    whole.close()
    for cuts in ([1] * 7, [2, 4, 1]):
        g, s, at, means, parts = None, 0, 0, [], []
        for m in cuts:
            acc = filled(grid, images, components, (at, m))
            g, s = acc.gram(region[at:at + m], g, s)
            a, b = acc.project(w, region[at:at + m], 1.25)
            means.append(a)
            parts.append(b)
            acc.close()
            at += m
        assert same(g, gram) and s == support, cuts
        assert same(np.concatenate(means), mean) and same(np.concatenate(parts, axis=1), modes), cuts


# ---- 8. the designed case ------------------------------------------------------------------------------------------------------

def test_designed_case_on_the_device():
    fields = R.designed_case()[0]
    chains = [field_chain(R.DESIGNED_GRID, f) for f in fields]
    for planes in (None, 4):
        res = group_modes(chains, R.DESIGNED_GRID, n_modes=4, max_planes=planes)
        assert res["support"].all() and res["n_support"] == 13 * 11 * 9
        check_designed(res["eigenvalues"], res["vectors"], res["mean"], res["modes"], res["n_support"], fields)
        assert np.abs(res["rms"][:3] / np.array(R.DESIGNED_SD) - 1).max() <= 2.0 ** -21 and abs(res["cumulative"][2] - 1) <= 2.0 ** -21
        if planes is None:
            whole = res
    for k in ("gram", "mean", "modes", "scores", "distance", "share"):
        assert same(res[k], whole[k]), k                    # three slabs change no bit


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals_come_before_the_device_is_touched():
    grid = unit_grid((5, 3, 2))
    lib = _abi.hip_lib()
    rng = np.random.default_rng(1)
    vols = rng.normal(size=(3, 2, 3, 5)).astype(F4)
    identity = Chain([Link.linear(np.eye(4))])
    f = np.empty(3 * 30 * 3, F4).ctypes.data_as(_abi.c_float_p)
    g = np.zeros(6, F8)
    gp, count = g.ctypes.data_as(_abi.c_double_p), C.c_uint64()
    w = np.ones(9, F8)
    wp = w.ctypes.data_as(_abi.c_double_p)
    one, three = ModeImages(grid, 3, 1), ModeImages(grid, 3, 3)
    src = one._views(vols[0])[1]
    # an add whose kind does not fit the components
    assert lib.frog_modes_add_displacement(one._h, identity._h, None, None) == _abi.FROG_E_INVALID
    assert lib.frog_modes_add_jacobian(three._h, identity._h, None, None, 0) == _abi.FROG_E_INVALID
    assert lib.frog_modes_add(three._h, None, src, None, 1, 0.0) == _abi.FROG_E_INVALID
    # what the frog_glm adds refuse: no chain, a float mask, a spacing of 0, a source of another size without a chain
    assert lib.frog_modes_add_displacement(three._h, None, None, None) == _abi.FROG_E_INVALID
    assert lib.frog_modes_add_jacobian(one._h, None, None, None, 0) == _abi.FROG_E_INVALID
    for call in (three.add_displacement, one.add_jacobian):
        for bad in (dict(mask=(np.ones((3, 3, 3), F4), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))), dict(support=((3, 3, 3), (0.0, 0.0, 0.0), (1.0, 0.0, 1.0)))):
            with pytest.raises(_abi.FrogError) as e:
                call(identity, **bad)
            assert e.value.code == _abi.FROG_E_INVALID, bad
    with pytest.raises(_abi.FrogError) as e:
        one.add(np.zeros((2, 3, 4), F4))
    assert e.value.code == _abi.FROG_E_INVALID
    assert lib.frog_modes_add(one._h, None, None, None, 1, 0.0) == _abi.FROG_E_INVALID
    # gram and project before n_images adds
    for k in range(2):
        one.add(vols[k])
        three.add_displacement(identity)
    for acc in (one, three):
        assert lib.frog_modes_gram(acc._h, None, gp, C.byref(count)) == _abi.FROG_E_INVALID
        assert lib.frog_modes_project(acc._h, None, 1, wp, 0.0, f, f) == _abi.FROG_E_INVALID
        assert lib.frog_modes_plane(acc._h, 2, f) == _abi.FROG_E_INVALID
    one.add(vols[2])
    three.add_displacement(identity)
    assert lib.frog_modes_add(one._h, None, src, None, 1, 0.0) == _abi.FROG_E_INVALID          # the fourth of three
    assert lib.frog_modes_add_displacement(three._h, identity._h, None, None) == _abi.FROG_E_INVALID
    for acc in (one, three):
        assert lib.frog_modes_gram(acc._h, None, gp, C.byref(count)) == _abi.FROG_OK
        assert lib.frog_modes_gram(acc._h, None, None, C.byref(count)) == _abi.FROG_E_INVALID and lib.frog_modes_gram(acc._h, None, gp, None) == _abi.FROG_E_INVALID
        assert lib.frog_modes_project(acc._h, None, 3, wp, 0.0, None, f) == _abi.FROG_OK     # the mean is optional
        for bad in (0, 4):
            assert lib.frog_modes_project(acc._h, None, bad, wp, 0.0, f, f) == _abi.FROG_E_INVALID, bad
        assert lib.frog_modes_project(acc._h, None, 1, None, 0.0, f, f) == _abi.FROG_E_INVALID and lib.frog_modes_project(acc._h, None, 1, wp, 0.0, f, None) == _abi.FROG_E_INVALID
        for bad in (np.nan, np.inf, -np.inf):
            w[4] = bad
            assert lib.frog_modes_project(acc._h, None, 2, wp, 0.0, f, f) == _abi.FROG_E_INVALID, bad
            assert lib.frog_modes_project(acc._h, None, 1, wp, 0.0, f, f) == _abi.FROG_OK            # beyond the first mode's weights
        w[4] = 1.0
        acc.close()
    assert count.value == 2 * 30                             # one good gram call per accumulator
    assert modes_planes(grid, 3, 3) == 2


# ---- 10. the tool --------------------------------------------------------------------------------------------------------------

def run(args, cwd, timeout=300):
    return subprocess.run(args, cwd=cwd, capture_output=True, text=True, timeout=timeout)


def directory(path):
    """Every file of a directory, the .nii.gz ones inflated."""
    return {name: gzip.decompress((path / name).read_bytes()) if name.endswith(".gz") else (path / name).read_bytes() for name in sorted(os.listdir(path))}


def test_group_modes_tool(tool_dir):
    d = tool_dir
    tool = [os.path.join(BIN, "GroupModes"), "bbox.json", SPACING]
    r = run(tool + ["-o", "modes_whole", "-k", "3", "-ms", "2"], d)
    assert r.returncode == 0 and "modes : 1 slab of 11 planes" in r.stdout, r.stdout + r.stderr
    r = run(tool + ["-o", "modes_slabs", "-k", "3", "-ms", "2", "-rp", "4"], d)
    assert r.returncode == 0 and "modes : 3 slabs of 4 planes" in r.stdout and "added twice" in r.stdout, r.stdout + r.stderr
    grid = bbox_grid(d / "bbox.json", float(SPACING))
    links = [invert(read_transform(d / "transforms" / f"{i}.json")) for i in range(N_TOOL)]
    res = group_modes([Chain(l) for l in links], grid, n_modes=3, mode_sd=2.0, max_planes=5)
    write_group_modes(res, grid, d / "modes_python", mode_sd=2.0)
    whole = directory(d / "modes_whole")
    names = ["mean.nii.gz", "support.nii.gz", "modes.csv", "scores.csv", "mean_field.nii.gz", "mean.json"]
    names += [f"mode_{k}{side}{ext}" for k in range(3) for side, ext in (("", ".nii.gz"), ("_plus", ".nii.gz"), ("_plus", ".json"), ("_minus", ".nii.gz"), ("_minus", ".json"))]
    assert sorted(whole) == sorted(names)
    assert directory(d / "modes_slabs") == whole and directory(d / "modes_python") == whole
    assert res["support"].all() and res["share"][0] > res["share"][1] > res["share"][2] > 0 and res["cumulative"][2] < 1
    assert read_volume(d / "modes_whole" / "support.nii.gz")[0].dtype == np.uint8
    table = (d / "modes_whole" / "scores.csv").read_text().splitlines()
    assert table[0] == "image,score_0,score_1,score_2,distance,distance_robust_z" and len(table) == 1 + N_TOOL
    assert (d / "modes_whole" / "modes.csv").read_text().splitlines()[0] == "mode,eigenvalue,rms,share,cumulative"
    # the scores of a mode are centred and have unit variance: it is in units per standard deviation
    b = np.array([[float(v) for v in line.split(",")[1:4]] for line in table[1:]])
    assert np.abs(b.mean(axis=0)).max() < 1e-12 and np.abs((b * b).sum(axis=0) / (N_TOOL - 1) - 1).max() < 1e-12
    # mode_0_plus.json through Chain moves every grid node by mean + 2 mode_0, to the float32 values the files hold
    dims, origin, spacing = grid
    moved = Chain(read_transform(d / "modes_whole" / "mode_0_plus.json")).sample(origin, spacing, dims, determinant=False, dtype=np.float64)[0]
    mean = read_nifti_lattice(d / "modes_whole" / "mean.nii.gz")[3].astype(F4)
    mode = read_nifti_lattice(d / "modes_whole" / "mode_0.nii.gz")[3].astype(F4)
    held = read_nifti_lattice(d / "modes_whole" / "mode_0_plus.nii.gz")[3].astype(F4)
    assert same(held, mean + F4(2.0) * mode) and same(mean.reshape(moved.shape), res["mean"])
    # node + value - node in float64 is the float32 value to a rounding unit of the node's coordinate (2^-46 at 60 mm)
    assert np.abs(moved.reshape(-1, 3) - held.astype(F8)).max() <= 2.0 ** -45
    # -nl 1: the chains without their linear links
    r = run(tool + ["-o", "modes_nl", "-k", "3", "-nl", "1", "-f", "-1"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    res = group_modes([Chain(drop_linear(l)) for l in links], grid, n_modes=3, fill=-1.0)
    write_group_modes(res, grid, d / "modes_nl_python")
    assert directory(d / "modes_nl") == directory(d / "modes_nl_python")
    assert not same(res["mean"], read_nifti_lattice(d / "modes_whole" / "mean.nii.gz")[3].astype(F4).reshape(res["mean"].shape))
    # scalar values
    r = run(tool + ["-o", "modes_jac", "-v", "logjacobian", "-k", "2"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    res = group_modes([Chain(l) for l in links], grid, "logjacobian", n_modes=2)
    write_group_modes(res, grid, d / "modes_jac_python")
    assert directory(d / "modes_jac") == directory(d / "modes_jac_python")
    # refused before anything is written
    for k, extra in enumerate((["-k", "0"], ["-k", "9"], ["-v", "volume"], ["-v", "images"], ["-nl", "2"], ["-ms", "-1"], ["-ms", "nan"],
                               ["-v", "jacobian", "-ms", "2"], ["-rp", "0"], ["-td", "nowhere"], ["-x", "1"])):
        r = run(tool + ["-o", f"modes_bad{k}"] + extra, d)
        assert r.returncode == 1 and "Error : " in r.stdout and not (d / f"modes_bad{k}").exists(), extra
