"""The transform tools' device kernels (frog_amd/csrc/device/chain.hip) pinned at their edges: every scalar type, rounding
ties, saturation, the half-voxel border, one-voxel-thick sources, points far outside a lattice, and launches of more than
2^32 work-items.  Sampling cases compare with volume_restate.reslice (reslice_voxel in NumPy f64, same operation order)
by np.array_equal, not a tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest

from frog_amd.chain import Chain, Link, invert
from frog_amd.volume import Average, average, read_volume, write_volume
from test_gpu_average import restate, same
from volume_restate import extreme_volume, reslice as restated

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

ALL_TYPES = ("uint8", "int8", "uint16", "int16", "uint32", "int32", "float32", "float64")
INT_TYPES = ALL_TYPES[:6]
EPS = 2.0 ** -30                    # a c this far past the border is outside

# a non-trivial affine map with fractional shifts, the source and an output grid that reaches past it
AFFINE = np.array([[0.75, 0.125, -0.0625, 1.3], [-0.05, 1.1, 0.03125, -0.7], [0.02, 0.0, 0.9, 0.37], [0.0, 0.0, 0.0, 1.0]])
SRC_SHAPE, SRC_O, SRC_S = (20, 24, 22), (-1.25, 0.5, 2.0), (1.5, 0.75, 1.25)
GRID = ((37, 33, 29), (-3.1, -0.4, 1.7), (1.1, 0.9, 1.3))


def _matrix_volumes():
    rng = np.random.default_rng(17)
    return {dt: extreme_volume(dt, SRC_SHAPE, rng) for dt in ALL_TYPES}


def device_outputs():
    """Every kernel of chain.hip on small inputs: the reslice matrix (8 types x 2 modes), apply and check through a B-spline
    chain and its inverse, the average of every type with and without a chain.  Also run in a child with the launch
    chunk forced small (test_small_launch_chunks_give_the_same_bytes)."""
    from test_chain import smooth_chain
    out = {}
    c = Chain([Link.linear(AFFINE)])
    for dt, vol in _matrix_volumes().items():
        for mode in (0, 1):
            out[f"reslice_{dt}_{mode}"] = c.reslice(vol, SRC_O, SRC_S, *GRID, mode, 3.0)
    links = smooth_chain()
    pts = np.random.default_rng(5).uniform(-30, 130, (5000, 3))
    for name, ch in (("fwd", Chain(links)), ("inv", Chain(invert(links)))):
        out[f"apply_{name}"] = ch.apply(pts)
        out[f"check_{name}"] = np.array(ch.check((-5.0, -5.0, -5.0), (2.5, 2.5, 2.5), (41, 40, 39)), np.float64)
    rng = np.random.default_rng(23)
    for dt in ALL_TYPES:
        vols = [extreme_volume(dt, (9, 10, 11), rng, huge_floats=False) for _ in range(3)]
        out[f"average_{dt}"] = np.stack(average(vols))
        chains = [Chain([Link.linear(AFFINE)]), Chain([]), Chain([Link.linear(np.diag([1.0, -1.0, 1.0, 1.0]))])]
        m, sd = average([(v, (0.5, -4.0, 0.25), (0.75, 1.0, 0.5)) for v in vols], chains, ((12, 9, 10), (-1.0, -3.0, 0.0), (0.5, 1.25, 0.5)), 1, 2.0)
        out[f"average_chain_{dt}"] = np.stack([m, sd])
    return out


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dtype", ALL_TYPES)
def test_reslice_every_type_equals_the_restatement(dtype, mode):
    vol = _matrix_volumes()[dtype]
    got = Chain([Link.linear(AFFINE)]).reslice(vol, SRC_O, SRC_S, *GRID, mode, 3.0)
    want = restated([Link.linear(AFFINE)], vol, SRC_O, SRC_S, *GRID, mode, 3.0)
    assert got.dtype == vol.dtype and got.shape == GRID[0][::-1]
    assert np.array_equal(got, want, equal_nan=True)
    bg = np.array(3.0).astype(dtype)
    assert (got == bg).mean() > 0.1 and (got != bg).mean() > 0.3            # both the source and the background are sampled
    if mode == 0 and dtype.startswith("float"):                              # nearest hands voxels through unchanged
        tiny = np.abs(got[got != 0]).min()
        assert tiny < np.finfo(dtype).tiny                                    # subnormals survive the round trip
    elif mode == 0:
        info = np.iinfo(dtype)
        assert (got == info.min).any() and (got == info.max).any()


def test_small_launch_chunks_give_the_same_bytes():
    """FROG_CHAIN_LAUNCH_MAX=1000 (read once per process: a child) = 768 work-items per launch: every kernel of chain.hip
    runs in many chunks, chain_check_kernel's block slots are indexed across them; same bytes as one launch."""
    code = ("import sys, numpy as np\n"
            "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_volume_edges as T\n"
            "np.savez(sys.argv[1], **T.device_outputs())\n") % (ROOT, HERE)
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), "frog_chain_chunks_%d.npz" % os.getpid())
    env = dict(os.environ, FROG_CHAIN_LAUNCH_MAX="1000")
    r = subprocess.run([sys.executable, "-c", code, path], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    chunked = dict(np.load(path))
    os.remove(path)
    plain = device_outputs()
    assert sorted(chunked) == sorted(plain) and len(plain) == 16 + 4 + 16
    for k, v in plain.items():
        assert v.dtype == chunked[k].dtype and v.tobytes() == chunked[k].tobytes(), k
    assert plain["check_fwd"][0] == 0 and np.isfinite(plain["check_fwd"][1])


def _ramps(dtype):
    info = np.iinfo(dtype)
    rows = [np.arange(int(info.min), int(info.min) + 8), np.arange(int(info.max) - 7, int(info.max) + 1),
            np.arange(-4, 4) if info.min < 0 else np.arange(0, 8)]
    if info.bits == 32:
        rows.append(np.arange(2 ** 24 - 3, 2 ** 24 + 5))                   # f32 cannot hold 2^24 + 1
        rows.append(np.arange(2 ** 32 - 260, 2 ** 32 - 252) if dtype == "uint32" else np.arange(2 ** 31 - 260, 2 ** 31 - 252))
    return [r.astype(dtype) for r in rows]


@pytest.mark.parametrize("dtype", INT_TYPES)
def test_ties_round_half_up(dtype):
    """Samples exactly halfway between neighbouring integers: linear gives k + 0.5 -> k + 1 (-2.5 -> -2, 2.5 -> 3), nearest
    at c = n + 0.5 reads voxel n + 1."""
    c = Chain([])
    grid = ((7, 2, 2), (0.5, 0.0, 0.0), (1.0, 1.0, 1.0))
    for row in _ramps(dtype):
        vol = np.broadcast_to(row, (2, 2, 8)).copy()
        lin = c.reslice(vol, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), *grid, 1, 0.0)
        near = c.reslice(vol, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), *grid, 0, 0.0)
        a, b = row[:-1].astype(np.float64), row[1:].astype(np.float64)
        assert np.array_equal(lin, np.broadcast_to(np.floor((a + b) / 2 + 0.5).astype(dtype), lin.shape)), row
        assert np.array_equal(near, np.broadcast_to(row[1:], near.shape)), row
        assert np.array_equal(lin, restated([], vol, (0, 0, 0), (1, 1, 1), *grid, 1, 0.0))
        assert np.array_equal(lin[0, 0], row[1:]), row                       # consecutive integers: every tie rounds up
    if np.iinfo(dtype).min < 0:
        lin = c.reslice(np.broadcast_to(np.array([-3, -2, 2, 3], dtype), (2, 2, 4)).copy(), (0, 0, 0), (1, 1, 1),
                        (2, 1, 1), (0.5, 0.0, 0.0), (2.0, 1.0, 1.0), 1, 0.0)
        assert lin[0, 0].tolist() == [-2, 3]                                 # -2.5 -> -2, 2.5 -> 3
    if dtype == "uint32":
        vol = np.broadcast_to(np.array([4294967294, 4294967295, 16777217, 16777218], np.uint32), (2, 2, 4)).copy()
        lin = c.reslice(vol, (0, 0, 0), (1, 1, 1), (2, 1, 1), (0.5, 0.0, 0.0), (2.0, 1.0, 1.0), 1, 0.0)
        assert lin[0, 0].tolist() == [4294967295, 16777218]


@pytest.mark.parametrize("dtype", INT_TYPES)
def test_background_saturates(dtype):
    info = np.iinfo(dtype)
    lo, hi = float(info.min), float(info.max)
    bgs = [lo - 5.0, hi + 5.0, lo - 0.5, hi + 0.49, lo - 0.51]
    if info.bits == 32:
        bgs += [-1e12, 1e12]
    vol = extreme_volume(dtype, (6, 7, 8), np.random.default_rng(3))
    grid = ((12, 11, 10), (-2.0, -1.5, -1.0), (1.0, 1.0, 1.0))
    for bg in bgs:
        for mode in (0, 1):
            got = Chain([]).reslice(vol, (0, 0, 0), (1, 1, 1), *grid, mode, bg)
            assert np.array_equal(got, restated([], vol, (0, 0, 0), (1, 1, 1), *grid, mode, bg)), (bg, mode)
            clamped = info.min if np.floor(bg + 0.5) <= lo else info.max
            assert got[0, 0, 0] == clamped and (got == clamped).mean() > 0.3, (bg, mode)


def _axis_line(dims, so, ss, axis, c_first, step):
    """An output grid with two samples along `axis`, at c = c_first and c_first + step, and the voxel centres on the others."""
    od, oo, os_ = list(dims), list(so), list(ss)
    od[axis] = 2
    oo[axis] = so[axis] + c_first * ss[axis]
    os_[axis] = step * ss[axis]
    return tuple(od), tuple(oo), tuple(os_)


@pytest.mark.parametrize("mode", [0, 1])
def test_half_voxel_border_on_each_axis(mode):
    """c = -0.5 and c = dims - 0.5 are inside and read the edge voxel; 2^-30 of a voxel further out is the background."""
    dims, so, ss = (5, 4, 3), (0.25, -1.0, 2.0), (0.5, 2.0, 1.25)
    c = Chain([])
    for dtype in ("int16", "uint32", "float64"):
        vol = (10 + np.arange(60)).reshape(dims[::-1]).astype(dtype)
        for axis in range(3):
            edges = np.take(vol, [0, dims[axis] - 1], axis=2 - axis)
            for c_first, step, inside in ((-0.5, dims[axis], True), (-0.5 - EPS, dims[axis] + 2 * EPS, False)):
                grid = _axis_line(dims, so, ss, axis, c_first, step)
                got = c.reslice(vol, so, ss, *grid, mode, 7.0)
                assert np.array_equal(got, restated([], vol, so, ss, *grid, mode, 7.0)), (dtype, axis, c_first)
                if inside:
                    assert np.array_equal(got, edges), (dtype, axis)
                else:
                    assert (got == 7).all(), (dtype, axis)


@pytest.mark.parametrize("thin_axis", [2, 1])
def test_one_voxel_thick_source(thin_axis):
    """sz = 1 (then sy = 1): within half a voxel of the slice every tap is the slice (linear: rz * A + fz * A = A for a
    dyadic shift and integer voxels); beyond it the background."""
    rng = np.random.default_rng(thin_axis)
    shape = [6, 7, 8]
    shape[2 - thin_axis] = 1
    dims, so, ss = tuple(shape[::-1]), (1.0, -2.0, 0.5), (0.75, 1.5, 2.0)
    c = Chain([])
    for dtype in ("uint16", "float32"):
        vol = (rng.integers(1, 60000, shape) if dtype == "uint16" else rng.normal(0, 100, shape)).astype(dtype)
        for off in (-0.75, -0.5 - EPS, -0.5, -0.3125, 0.0, 0.375, 0.5, 0.5 + EPS, 1.0):
            od, oo, os_ = list(dims), list(so), list(ss)
            oo[thin_axis] = so[thin_axis] + off * ss[thin_axis]
            for mode in (0, 1):
                got = c.reslice(vol, so, ss, od, oo, os_, mode, 9.0)
                assert np.array_equal(got, restated([], vol, so, ss, od, oo, os_, mode, 9.0)), (dtype, off, mode)
                if abs(off) > 0.5:
                    assert (got == 9).all()
                elif dtype == "uint16" or mode == 0 or off in (0.0, -0.5, 0.5):
                    assert np.array_equal(got, vol), (dtype, off, mode)


@pytest.mark.parametrize("n_images", [1, 3])
def test_average_every_type(n_images):
    """Average / average of every scalar type, with and without chains, equal to the restatement of AverageVolumes over the
    per-image Chain.reslice volumes (themselves equal to the reslice restatement).  One image: mean = float32(v), stdev 0."""
    rng = np.random.default_rng(40 + n_images)
    grid = ((12, 9, 10), (-1.0, -3.0, 0.0), (0.5, 1.25, 0.5))
    so, ss = (0.5, -4.0, 0.25), (0.75, 1.0, 0.5)
    mats = [AFFINE, np.diag([1.0, -1.0, 1.0, 1.0]) + np.array([[0, 0, 0, 0.25], [0, 0, 0, 0.5], [0, 0, 0, -0.125], [0, 0, 0, 0]])]
    for dtype in ALL_TYPES:
        vols = [extreme_volume(dtype, (9, 10, 11), rng, huge_floats=False) for _ in range(n_images)]
        m, sd = average(vols)
        wm, ws = restate(vols)
        assert same(m, wm) and same(sd, ws), dtype
        if n_images == 1:
            assert same(m, vols[0].astype(np.float32)) and (sd == 0).all(), dtype
        links = [[Link.linear(mats[k % 2])] for k in range(n_images)]
        per = [Chain(l).reslice(v, so, ss, *grid, 1, 2.0) for l, v in zip(links, vols)]
        for l, v, r in zip(links, vols, per):
            assert np.array_equal(r, restated(l, v, so, ss, *grid, 1, 2.0)), dtype
        acc = Average(grid, n_images)
        for l, v, r in zip(links, vols, per):
            assert same(acc.add((v, so, ss), Chain(l), 1, 2.0, resliced=True), r), dtype
        m, sd = acc.finish()
        wm, ws = restate(per)
        assert same(m, wm) and same(sd, ws), dtype
        if n_images == 1:
            assert same(m, per[0].astype(np.float32)) and (sd == 0).all(), dtype


def test_points_far_outside_a_lattice():
    """A point 1e12 or 1e15 mm out on one axis is outside every lattice: the forward link and its Newton inverse return it
    unchanged (border = zero).  A NaN coordinate gives NaN there and no finite wrong value anywhere."""
    from oracle.oracle_api import chain_apply
    from test_chain import smooth_chain
    lattice = [smooth_chain()[1]]
    base = np.array([10.0, 20.0, 30.0])
    far, nan = [], []
    for axis in range(3):
        for v in (1e12, -1e12, 1e15, -1e15):
            p = base.copy(); p[axis] = v
            far.append(p)
        p = base.copy(); p[axis] = np.nan
        nan.append(p)
    far, nan = np.array(far), np.array(nan)
    for links in (lattice, invert(lattice)):
        c = Chain(links)
        assert np.array_equal(c.apply(far), far) and np.array_equal(chain_apply(links, far), far)
        for got in (c.apply(nan), chain_apply(links, nan)):
            assert np.isnan(got[np.isnan(nan)]).all()
            assert ((got == nan) | np.isnan(got)).all()
        assert not np.array_equal(c.apply(base[None]), base[None])        # the lattice does move points inside it


def test_check_over_more_than_2_32_nodes():
    """frog_chain_check over 2^32 + 2^20 nodes (65536 x 65552 x 1): three launches of at most 2^31 work-items, 16.8 M block
    slots (134 MB on the device and the host).  A mirror has determinant -1 at every node, the identity 1."""
    dims = (65536, 65552, 1)
    total = dims[0] * dims[1] * dims[2]
    assert total == 2 ** 32 + 2 ** 20
    mirror = Chain([Link.linear(np.diag([-1.0, 1.0, 1.0, 1.0]))])
    assert mirror.check((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), dims) == (total, -1.0)
    assert Chain([]).check((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), dims) == (0, 1.0)


def test_reslice_onto_more_than_2_32_voxels():
    """A u8 source of 65536 x 257 onto 65536 x 65537 voxels (2^32 + 2^16): 4.3 GB on the device and 4.3 GB of host output,
    verified slab by slab (128 MB at a time).  Output voxel (i, j) reads source (i + 3, round(j / 256)), nearest; the last
    three columns are the background 7.  No output voxel is 0, so a tail left unwritten shows."""
    sx, sy = 65536, 257
    x = np.arange(sx, dtype=np.int64)
    src = (8 + (x[None, :] * 7 + np.arange(sy, dtype=np.int64)[:, None] * 13) % 240).astype(np.uint8)[None]
    M = np.array([[1.0, 0, 0, 3.0], [0, 1.0 / 256, 0, 0], [0, 0, 1.0, 0], [0, 0, 0, 1.0]])
    nx, ny = 65536, 65537
    out = Chain([Link.linear(M)]).reslice(src, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (nx, ny, 1), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 0, 7.0)
    assert out.shape == (1, ny, nx) and nx * ny == 2 ** 32 + 2 ** 16
    rows = 2048
    for j0 in range(0, ny, rows):
        j = np.arange(j0, min(ny, j0 + rows))
        want = np.full((len(j), nx), 7, np.uint8)
        want[:, :nx - 3] = src[0, np.floor(j / 256 + 0.5).astype(np.int64), 3:]
        assert np.array_equal(out[0, j0:j0 + len(j)], want), j0
    tail = out.reshape(-1)[2 ** 32:]                                           # the work-items past 2^32
    assert len(tail) == 2 ** 16 and np.array_equal(tail[:nx - 3], src[0, 256, 3:]) and (tail[nx - 3:] == 7).all()


def test_volume_transform_tool_keeps_the_type_and_saturates(tmp_path):
    """bin/VolumeTransform on a uint16 .nii.gz and an int8 .mhd with -b outside the type's range: the file it writes equals
    Chain(invert(links)).reslice bit for bit, in the source's type, on the reference's grid."""
    from test_chain import smooth_chain
    from test_gpu_chain import _write_chain
    links = smooth_chain()
    _write_chain(tmp_path / "t.json", links)
    rd = (36, 30, 28)
    write_volume(tmp_path / "ref.mhd", np.zeros(rd[::-1], np.uint8), (0.0, 1.0, 2.0), (2.0, 2.0, 2.5))
    _, ro, rs = read_volume(tmp_path / "ref.mhd")
    z, y, x = np.meshgrid(np.arange(40), np.arange(48), np.arange(56), indexing="ij")
    wave = np.sin(x / 6.0) * np.cos(y / 7.0)
    inv = Chain(invert(links))
    for name, vol, args, mode, bg in (("src.nii.gz", (32000 + 33000 * wave + 10 * z).clip(0, 65535).astype(np.uint16), [], 1, 70000.0),
                                      ("src.mhd", (127 * wave).astype(np.int8), ["-i", "0"], 0, -1000.0)):
        write_volume(tmp_path / name, vol, (-4.0, -2.0, 0.0), (1.5, 1.5, 2.0))
        src, so, ss = read_volume(tmp_path / name)
        assert src.dtype == vol.dtype and np.array_equal(src, vol)
        r = subprocess.run([os.path.join(ROOT, "bin", "VolumeTransform"), name, "ref.mhd", "-t", "t.json", "-b", repr(bg), "-o", "out_" + name] + args,
                           cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        got, o, s = read_volume(tmp_path / ("out_" + name))
        want = inv.reslice(src, so, ss, rd, ro, rs, mode, float(np.float32(bg)))
        assert got.dtype == vol.dtype and o == ro and s == rs
        assert same(got, want), name
        info = np.iinfo(vol.dtype)
        assert (got == (info.max if bg > 0 else info.min)).any() and (got != got.flat[0]).any()      # the source never holds it
