"""frog_chain_sample (dense displacement field + Jacobian determinant map of a transform chain), the FROG_T_FIELD link that
takes such a field back into a chain, and bin/TransformField: against the CPU oracle, against frog_chain_check bit for bit,
against the NumPy restatement (tests/field_restate.py) bit for bit, and on closed forms."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from field_restate import affine_sample, field_apply, node_list
from frog_amd import _abi
from frog_amd.chain import FIELD, Chain, Link, invert, read_transform
from oracle.oracle_api import chain_apply
from test_chain import linear_lattice, smooth_chain
from test_gpu_chain import _write_chain, random_chain

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = ((-5.0, -5.0, -5.0), (2.5, 2.5, 2.5), (41, 40, 39))              # the grid of test_gpu_chain: 63960 nodes, not a multiple of 256


def chains_for_the_exact_checks():
    rng = np.random.default_rng(7)
    smooth, wild = random_chain(rng, 3, 0.5), random_chain(rng, 3, 20.0)
    return {"smooth": smooth, "wild": wild, "inverse": invert(smooth), "empty": []}


# ---- 1. against the oracle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("amplitude", [0.5, 20.0])
def test_sample_matches_oracle(amplitude):
    links = random_chain(np.random.default_rng(7), 3, amplitude)
    nodes = node_list(*GRID)
    want, J = chain_apply(links, nodes, jacobian=True)
    want_disp, want_det = want - nodes, np.linalg.det(J)
    disp, det = Chain(links).sample(*GRID, dtype=np.float64)
    assert disp.shape == (39, 40, 41, 3) and det.shape == (39, 40, 41) and disp.dtype == det.dtype == np.float64
    e_disp, e_det = np.abs(disp.reshape(-1, 3) - want_disp).max(), np.abs(det.ravel() - want_det).max()
    print(f"amplitude {amplitude}: displacement error {e_disp:.3e} (max |d| {np.abs(want_disp).max():.3g}), "
          f"determinant error {e_det:.3e} (max |det| {np.abs(want_det).max():.3g})")
    assert e_disp < 1e-9 * max(1.0, np.abs(want_disp).max())
    assert e_det < 1e-9 * max(1.0, np.abs(want_det).max())
    assert (det < 0).any() == (amplitude > 1)


def test_sampled_inverse_composes_with_the_chain_to_the_identity():
    links = random_chain(np.random.default_rng(7), 3, 0.5)
    nodes = node_list(*GRID)
    disp, det = Chain(invert(links)).sample(*GRID, dtype=np.float64)
    back = Chain(links).apply(nodes + disp.reshape(-1, 3))
    err = np.abs(back - nodes).max()
    print(f"forward(node + sampled inverse displacement) - node: {err:.3e} mm")
    assert err < 2e-3                                                   # the tolerance the Newton inverse iterates to
    assert (det > 0).all()


# ---- 2. against frog_chain_check, exactly --------------------------------------------------------------------------------
def exact_checks(name, links, grid):
    """Everything section 2 of the feature asks, on one chain and grid; returns the four arrays."""
    c = Chain(links)
    n, m = c.check(*grid)
    d64, j64 = c.sample(*grid, dtype=np.float64)
    d32, j32 = c.sample(*grid, dtype=np.float32)
    assert int((j64 < 0).sum()) == n and j64.min() == m, (name, n, m, int((j64 < 0).sum()), j64.min())
    assert d32.dtype == j32.dtype == np.float32
    assert np.array_equal(j32, j64.astype(np.float32)) and np.array_equal(d32, d64.astype(np.float32)), name
    for dt, d, j in ((np.float64, d64, j64), (np.float32, d32, j32)):
        only_d, none = c.sample(*grid, determinant=False, dtype=dt)
        assert none is None and np.array_equal(only_d, d), name
        none, only_j = c.sample(*grid, displacement=False, dtype=dt)
        assert none is None and np.array_equal(only_j, j), name
    return d64, j64, d32, j32


def test_sample_equals_check_bit_for_bit(tmp_path):
    results = {}
    for name, links in chains_for_the_exact_checks().items():
        results[name] = exact_checks(name, links, GRID)
    assert (results["wild"][1] < 0).sum() > 100 and (results["smooth"][1] > 0).all()
    assert not results["empty"][0].any() and (results["empty"][1] == 1.0).all()
    # once more in a fresh process whose launches hold 512 nodes (the variable is read once per process): 125 launches in
    # 32 slabs, the last one partial, must give the same bits
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import numpy as np\n"
            "import test_gpu_field as t\n"
            "out = {}\n"
            "for name, links in t.chains_for_the_exact_checks().items():\n"
            "    for k, a in enumerate(t.exact_checks(name, links, t.GRID)):\n"
            "        out[name + str(k)] = a\n"
            "np.savez(sys.argv[1], **out)\n" % (ROOT, os.path.join(ROOT, "tests")))
    env = dict(os.environ, FROG_CHAIN_LAUNCH_MAX="512")
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path / "child.npz")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    child = np.load(tmp_path / "child.npz")
    for name, arrays in results.items():
        for k, a in enumerate(arrays):
            assert np.array_equal(child[name + str(k)], a), (name, k)


# ---- 3. bit for bit on affine chains -------------------------------------------------------------------------------------
def test_affine_chains_equal_the_restatement_bit_for_bit():
    rng = np.random.default_rng(21)
    M1 = np.eye(4); M1[:3, :3] = np.eye(3) + rng.normal(0, 0.2, (3, 3)); M1[:3, 3] = rng.uniform(-7, 7, 3)
    M2 = np.eye(4); M2[:3, :3] = np.diag([1.3, -0.7, 0.9]) + rng.normal(0, 0.1, (3, 3)); M2[:3, 3] = [0.1, -33.3, 1e-3]
    grids = [((0.1, -0.7, 3.3), (0.3, 1.7, 0.9), (37, 23, 11)), ((-12.345, 1e-3, 1e3 / 3), (1 / 3, 0.07, 2.5), (7, 129, 5))]
    for links in ([Link.linear(M1)], [Link.linear(M1), Link.linear(M2)], [Link.linear(M2), Link.linear(M1)]):
        c = Chain(links)
        for grid in grids:
            want_d, want_j = affine_sample(links, *grid)
            disp, det = c.sample(*grid, dtype=np.float64)
            assert np.array_equal(disp, want_d) and np.array_equal(det, want_j)
            d32, j32 = c.sample(*grid)
            assert d32.dtype == np.float32 and np.array_equal(d32, want_d.astype(np.float32)) and np.array_equal(j32, want_j.astype(np.float32))
            assert abs(det[0, 0, 0] - np.prod([np.linalg.det(l.matrix[:3, :3]) for l in links])) < 1e-12


# ---- 4. closed forms ------------------------------------------------------------------------------------------------------
def test_closed_forms():
    A = np.array([[0.25, 0, 0], [0, 0, -0.5], [0.1, 0.2, 0]])
    t = np.array([1.0, -2.0, 0.5])
    L = linear_lattice((9, 8, 10), (-12.0, -10.0, -15.0), (5.0, 4.0, 6.0), A, t)
    grid = ((-2.0, -2.0, -2.0), (1.0, 1.0, 1.0), (12, 12, 12))         # interior: all 64 taps exist
    nodes = node_list(*grid)
    disp, det = Chain([L]).sample(*grid, dtype=np.float64)
    assert np.allclose(disp.reshape(-1, 3), nodes @ A.T + t, rtol=0, atol=1e-5)
    assert np.abs(det - np.linalg.det(np.eye(3) + A)).max() < 1e-6
    fold = linear_lattice((10, 10, 10), (-20.0, -20.0, -20.0), (5.0, 5.0, 5.0), np.diag([-1.5, 0.0, 0.0]), [0, 0, 0])
    _, det = Chain([fold]).sample((-6.0, -6.0, -6.0), (1.0, 1.0, 1.0), (12, 11, 10))
    assert det.shape == (10, 11, 12) and (det < 0).all() and np.abs(det + 0.5).max() < 1e-6


# ---- 5. the field link ----------------------------------------------------------------------------------------------------
def random_field(rng, dims, origin, spacing, amplitude=3.0):
    return Link.field(dims, origin, spacing, (amplitude * rng.normal(size=(dims[0] * dims[1] * dims[2], 3))).astype(np.float32))


def test_field_link_returns_its_nodes_exactly():
    # dyadic origin and spacing: (p - origin) / spacing is the node's index exactly, so every fraction is 0 or 1 and
    # 1 * a + 0 * b is exact for finite values
    grid = ((-3.5, 2.25, 0.0), (1.5, 2.0, 0.75), (7, 6, 5))
    f = random_field(np.random.default_rng(31), grid[2], grid[0], grid[1])
    nodes = node_list(*grid)
    got = Chain([f]).apply(nodes)
    assert np.array_equal(got, nodes + f.coeffs.astype(np.float64))
    assert np.array_equal(got, field_apply(f, nodes))


@pytest.mark.parametrize("dims", [(9, 7, 8), (5, 1, 4), (1, 1, 3)])
def test_field_link_equals_the_restatement_inside_and_outside(dims):
    rng = np.random.default_rng(32)
    origin, spacing = (-3.3, 0.7, 10.1), (1.3, 0.9, 2.7)
    f = random_field(rng, dims, origin, spacing)
    lo = np.array(origin); hi = lo + (np.array(dims) - 1) * np.array(spacing)
    pts = [rng.uniform(lo, hi, (4000, 3))]
    for axis in range(3):                                               # beyond each face, the other axes inside
        for side in (-1, 1):
            p = rng.uniform(lo, hi, (300, 3))
            p[:, axis] = (lo[axis] - rng.uniform(0.01, 50, 300)) if side < 0 else (hi[axis] + rng.uniform(0.01, 50, 300))
            pts.append(p)
    pts.append(rng.uniform(lo - 40, hi + 40, (1000, 3)))                # corners and edges
    pts.append(node_list(origin, spacing, dims))
    pts.append(np.array([[1e300, -1e300, 0.0], [np.inf, 0.0, -np.inf]]))
    pts = np.concatenate(pts)
    c = Chain([f])
    got = c.apply(pts)
    assert np.array_equal(got, field_apply(f, pts))
    # two field links in a row, and one behind a matrix: the chain composes them like any other link
    M = np.eye(4); M[:3, :3] += rng.normal(0, 0.1, (3, 3)); M[:3, 3] = [0.5, -1.0, 2.0]
    g = random_field(rng, (4, 5, 6), (-2.0, 0.0, 9.0), (3.1, 1.9, 2.2))
    q = pts[:4000]
    lin = (np.stack([M[r, 0] * q[:, 0] + M[r, 1] * q[:, 1] + M[r, 2] * q[:, 2] + M[r, 3] for r in range(3)], -1))
    assert np.array_equal(Chain([Link.linear(M), f, g]).apply(q), field_apply(g, field_apply(f, lin)))
    # a NaN coordinate gives NaN
    bad = np.array([[np.nan, 1.0, 11.0], [0.0, np.nan, 11.0], [0.0, 1.0, np.nan]])
    assert np.isnan(c.apply(bad)).all()
    # the analytic Jacobian against the restatement's, on a grid that straddles the field's: the determinant map
    sgrid = (tuple(lo - 2.0), (0.37, 0.41, 0.53), (40, 30, 50))
    _, J = field_apply(f, node_list(*sgrid), jacobian=True)
    want = np.linalg.det(J)
    _, det = c.sample(*sgrid, dtype=np.float64)
    assert np.abs(det.ravel() - want).max() < 1e-12 * max(1.0, np.abs(want).max())
    n, m = c.check(*sgrid)
    assert n == int((det < 0).sum()) and m == det.min()


def test_linear_field_has_the_constant_determinant():
    # d(p) = A p + t with small dyadic A, t on an integer grid: every node value is an f32 exactly, the interpolant is the
    # linear map itself, so inside the field's grid the determinant is det(I + A) up to the rounding of a few f64 operations
    A = np.array([[0.25, -0.125, 0.0], [0.5, 0.0, 0.0625], [0.0, 0.375, -0.25]])
    t = np.array([1.5, -0.75, 2.0])
    dims, origin, spacing = (12, 10, 11), (-4.0, -3.0, -5.0), (1.0, 1.0, 1.0)
    nodes = node_list(origin, spacing, dims)
    values = nodes @ A.T + t
    assert np.array_equal(values.astype(np.float32).astype(np.float64), values)
    f = Link.field(dims, origin, spacing, values)
    c = Chain([f])
    inner = ((-3.5, -2.75, -4.5), (0.25, 0.3, 0.7), (40, 29, 13))       # within [-4, 7] x [-3, 6] x [-5, 5]
    n, m = c.check(*inner)
    assert n == 0 and abs(m - np.linalg.det(np.eye(3) + A)) < 1e-12
    _, det = c.sample(*inner, dtype=np.float64)
    assert np.abs(det - np.linalg.det(np.eye(3) + A)).max() < 1e-12
    pts = np.random.default_rng(33).uniform([-4, -3, -5], [7, 6, 5], (2000, 3))
    assert np.abs(c.apply(pts) - (pts + pts @ A.T + t)).max() < 1e-12
    # outside the grid the clamped axis' column is zero: beyond +x the determinant is that of I + A without A's first column
    outer = ((8.0, -2.0, -4.0), (1.0, 1.0, 1.0), (3, 4, 5))
    B = np.eye(3) + A; B[:, 0] = [1, 0, 0]
    _, det = c.sample(*outer, dtype=np.float64)
    assert np.abs(det - np.linalg.det(B)).max() < 1e-12


def test_zero_field_reslices_like_the_empty_chain():
    rng = np.random.default_rng(34)
    zero = Link.field((6, 5, 4), (0.0, 0.0, 0.0), (7.0, 9.0, 11.0), np.zeros((120, 3), np.float32))
    o, s = (-5.0, 0.0, 2.0), (1.5, 2.0, 1.0)
    for dtype in ("int16", "float32", "uint8"):
        vol = rng.uniform(0, 200, (20, 30, 25)).astype(dtype)
        for mode in (0, 1):
            args = (vol, o, s, (33, 35, 31), (-7.0, 2.0, 4.0), (1.3, 1.5, 0.7), mode, 3.0)
            assert np.array_equal(Chain([zero]).reslice(*args), Chain([]).reslice(*args))


def test_validation():
    c = Chain([Link.linear(np.eye(4))])
    lib = _abi.hip_lib()
    o = (C.c_double * 3)(0, 0, 0); s = (C.c_double * 3)(1, 1, 1); d = (C.c_uint32 * 3)(2, 2, 2)
    out = np.full(8 * 3, 7.0, np.float64)
    p = out.ctypes.data
    F32, F64 = 6, 7
    for args in ((c._h, None, s, d, F32, p, None), (c._h, o, None, d, F32, p, None), (c._h, o, s, None, F32, p, None),
                 (c._h, o, s, d, F32, None, None), (c._h, o, s, d, 3, p, None), (c._h, o, s, d, 8, None, p)):
        assert lib.frog_chain_sample(*args) == _abi.FROG_E_INVALID and lib.frog_last_error()
    big = (C.c_uint32 * 3)(1 << 20, 1 << 20, 2)                          # 2^41 nodes
    assert lib.frog_chain_sample(c._h, o, s, big, F64, None, p) == _abi.FROG_E_INVALID and b"too large" in lib.frog_last_error()
    huge = (C.c_uint32 * 3)(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)          # the product wraps around 2^64
    assert lib.frog_chain_sample(c._h, o, s, huge, F64, None, p) == _abi.FROG_E_INVALID
    for dims in ((0, 5, 5), (5, 0, 5), (5, 5, 0)):                       # no nodes: nothing written
        assert lib.frog_chain_sample(c._h, o, s, (C.c_uint32 * 3)(*dims), F64, p, None) == _abi.FROG_OK
    assert (out == 7.0).all()
    with pytest.raises(ValueError):
        c.sample((0, 0, 0), (1, 1, 1), (2, 2, 2), dtype=np.int32)
    with pytest.raises(RuntimeError):
        c.sample((0, 0, 0), (1, 1, 1), (2, 2, 2), displacement=False, determinant=False)
    disp, det = c.sample((0, 0, 0), (0, 0, 0), (2, 2, 2))               # the grid's spacing is not validated
    assert not disp.any() and (det == 1).all()
    # a field link is validated like a lattice
    z = np.zeros((8, 3), np.float32)
    with pytest.raises(RuntimeError):
        Chain([Link.field((2, 2, 2), (0, 0, 0), (1, 0, 1), z)])
    with pytest.raises(RuntimeError):
        Chain([Link.field((2, 2, 2), (0, 0, 0), (1, -1, 1), z)])
    with pytest.raises(RuntimeError):
        Chain([Link.field((0, 2, 2), (0, 0, 0), (1, 1, 1), np.zeros((0, 3), np.float32))])


# ---- 6. collapse: a chain sampled into one field link ---------------------------------------------------------------------
def test_collapsed_chain_converges_at_second_order():
    """The finest lattice of random_chain(rng, 3, .) has a spacing of 5: h = 1.25 is a quarter of it.  Trilinear
    interpolation of a C2 function has an error bound proportional to h^2, so halving h must at least halve the largest error."""
    rng = np.random.default_rng(7)
    links = random_chain(rng, 3, 0.5)
    c = Chain(links)
    pts = rng.uniform(0.0, 100.0, (5000, 3))
    want = c.apply(pts)
    errors = []
    for h, n in ((1.25, 81), (0.625, 161)):                             # the same extent [0, 100]^3
        grid = ((0.0, 0.0, 0.0), (h, h, h), (n, n, n))
        disp, _ = c.sample(*grid, determinant=False)
        field = Link.field(grid[2], grid[0], grid[1], disp)
        errors.append(np.abs(Chain([field]).apply(pts) - want).max())
    print(f"collapse error: h = 1.25: {errors[0]:.4e} mm, h = 0.625: {errors[1]:.4e} mm, ratio {errors[0] / errors[1]:.2f}")
    assert errors[1] * 2 <= errors[0]


# ---- 7. bin/TransformField end to end --------------------------------------------------------------------------------------
def run(exe, args, cwd):
    return subprocess.run([os.path.join(ROOT, "bin", exe)] + args, cwd=cwd, capture_output=True, text=True, timeout=300)


def negatives(stdout):
    return int(stdout.split(" negative jacobian determinant values")[0].split()[-1])


@pytest.mark.parametrize("resize", [None, "2"])
def test_tool_transform_field(tmp_path, resize):
    from frog_amd.volume import read_volume, write_volume
    from nifti_util import read_nifti
    lib = _abi.host_lib()
    links = random_chain(np.random.default_rng(5), 2, 8.0)              # wild enough to fold in places
    _write_chain(tmp_path / "t.json", links)
    dims, origin, spacing = (30, 28, 26), (-3.0, 2.0, 1.0), (2.0, 2.5, 3.0)      # f32 values, as the headers store them
    d = (C.c_uint32 * 3)(*dims); s = (C.c_double * 3)(*spacing); o = (C.c_double * 3)(*origin)
    assert lib.frog_nifti_write(str(tmp_path / "vol.nii.gz").encode(), d, s, o, 1, np.zeros(30 * 28 * 26, np.float32).ctypes.data_as(_abi.c_float_p)) == 0
    extra = ["-s", resize] if resize else []
    if resize:
        sp = float(resize)
        dims = tuple(int(max(1.0, np.floor(n * v / sp + 0.5))) for n, v in zip(dims, spacing))       # CheckDiffeomorphism's rule
        assert dims == (30, 35, 39)
        spacing = (sp, sp, sp)
    r = run("TransformField", ["vol.nii.gz", "-t", "t.json"] + extra + ["-o", "f.nii.gz", "-j", "j.nii.gz", "-w", "c.json"], tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    want_d, want_j = Chain(links).sample(origin, spacing, dims, dtype=np.float32)
    for name, want, nc in (("f.nii.gz", want_d.reshape(-1, 3), 3), ("j.nii.gz", want_j.reshape(-1, 1), 1)):
        h, vox = read_nifti(tmp_path / name)
        assert tuple(h["dim"][1:4]) == dims and h["pixdim"][1:4] == spacing and h["qoffset"] == origin and h["datatype"] == 16
        assert vox.shape == (dims[0] * dims[1] * dims[2], nc) and np.array_equal(vox, want)
    chk = run("CheckDiffeomorphism", ["vol.nii.gz", "t.json"] + ([resize] if resize else []), tmp_path)
    n = negatives(r.stdout)
    assert n == negatives(chk.stdout) == int((want_j < 0).sum()) and n > 0
    assert ("Resizing image with spacing : 2" in r.stdout) == bool(resize)
    lo, hi = (float(v) for v in r.stdout.split("jacobian determinant range :")[1].split()[:2])
    j64 = Chain(links).sample(origin, spacing, dims, displacement=False, dtype=np.float64)[1]
    assert abs(lo - j64.min()) <= 1e-8 * abs(j64.min()) and abs(hi - j64.max()) <= 1e-8 * abs(j64.max())
    # the written chain: one field link that returns the written displacements at its nodes
    assert json.load(open(tmp_path / "c.json")) == {"transforms": [{"type": "frogDisplacementField", "file": "f.nii.gz"}]}
    back = read_transform(tmp_path / "c.json")
    assert len(back) == 1 and back[0].kind == FIELD and back[0].dims == dims and back[0].origin == origin and back[0].spacing == spacing
    nodes = node_list(origin, spacing, dims)
    assert np.array_equal(Chain(back).apply(nodes), nodes + want_d.reshape(-1, 3).astype(np.float64))
    # ... and feeds VolumeTransform -ti and PointsTransform -t directly
    z, y, x = np.meshgrid(np.arange(40), np.arange(48), np.arange(56), indexing="ij")
    src = (1000 + 400 * np.sin(x / 6.0) * np.cos(y / 7.0) + 10 * z).astype(np.int16)
    so, ss = (-4.0, -2.0, 0.0), (1.5, 1.5, 2.0)
    write_volume(tmp_path / "src.nii.gz", src, so, ss)
    r = run("VolumeTransform", ["src.nii.gz", "vol.nii.gz", "-ti", "c.json", "-o", "out.nii.gz"], tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    got, go, gs = read_volume(tmp_path / "out.nii.gz")
    want = Chain(back).reslice(src, so, ss, (30, 28, 26), (-3.0, 2.0, 1.0), (2.0, 2.5, 3.0), 1, float(src.min()))
    assert got.dtype == np.int16 and np.array_equal(got, want) and (got != src.min()).mean() > 0.3
    r = run("PointsTransform", ["-p", "20", "15", "30", "-t", "c.json"], tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    got = [float(v) for v in r.stdout.split("Output point :")[1].split()[:3]]
    assert np.allclose(got, Chain(back).apply([[20.0, 15.0, 30.0]])[0], rtol=1e-5)
    # a field link cannot be inverted: VolumeTransform -t says so and fails
    r = run("VolumeTransform", ["src.nii.gz", "vol.nii.gz", "-t", "c.json", "-o", "no.nii.gz"], tmp_path)
    assert r.returncode != 0 and "no inverse form" in r.stdout and not (tmp_path / "no.nii.gz").exists()


def test_tool_writes_the_inverse_as_a_field(tmp_path):
    """-ti: the inverted chain sampled once; the field then stands for the Newton inverse (VolumeTransform -t's chain)."""
    lib = _abi.host_lib()
    links = smooth_chain()
    _write_chain(tmp_path / "t.json", links)
    dims, origin, spacing = (24, 20, 22), (0.0, 1.0, 2.0), (2.0, 2.0, 2.5)
    d = (C.c_uint32 * 3)(*dims); s = (C.c_double * 3)(*spacing); o = (C.c_double * 3)(*origin)
    assert lib.frog_nifti_write(str(tmp_path / "ref.nii").encode(), d, s, o, 1, np.zeros(24 * 20 * 22, np.float32).ctypes.data_as(_abi.c_float_p)) == 0
    r = run("TransformField", ["ref.nii", "-ti", "t.json", "-o", "inv.nii.gz", "-w", "inv.json"], tmp_path)
    assert r.returncode == 0 and "0 negative jacobian determinant values (0%)" in r.stdout, r.stdout + r.stderr
    assert not (tmp_path / "j.nii.gz").exists()
    field = read_transform(tmp_path / "inv.json")
    want, _ = Chain(invert(links)).sample(origin, spacing, dims, determinant=False)
    assert np.array_equal(field[0].coeffs, want.reshape(-1, 3))
    nodes = node_list(origin, spacing, dims)
    assert np.abs(Chain(links).apply(Chain(field).apply(nodes)) - nodes).max() < 2e-3
