"""The coverage-aware group average on the device (frog_cover, include/frog_chain.h; frog_amd.volume.CoverAverage;
bin/AverageImage -c 1) against its NumPy restatement (cover_restate.py).  Every comparison is == on bits; NaN patterns go
through an integer view."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from frog_amd import _abi
from frog_amd.chain import Chain, Link, invert, read_transform
from frog_amd.volume import CoverAverage, average, bbox_grid, cover_average, read_volume, write_volume

import cover_restate
from volume_restate import extreme_volume

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.path.join(ROOT, "bin")

ALL_TYPES = ("uint8", "int8", "uint16", "int16", "uint32", "int32", "float32", "float64")
GRID = ((19, 17, 13), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))     # 4199 voxels: seventeen blocks of 256, the last one partial
SRC_SHAPE, SRC_S = (10, 11, 12), (1.0, 1.0, 1.0)            # 12 x 11 x 10 voxels
# where each source's first voxel lies on the grid, and a fractional (dyadic) linear part per image
OFFSETS = ((0.3, 0.2, 0.1), (2.6, 1.7, 0.9), (4.4, 3.3, 1.6), (6.7, 5.1, 2.8), (3.5, 2.5, 1.2))
TILTS = ((0.0, 0.0, 0.0), (0.03125, -0.015625, 0.0), (-0.0625, 0.0, 0.03125), (0.0, 0.046875, -0.03125), (0.015625, 0.03125, 0.0625))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def same3(got, want):
    return all(same(g, w) for g, w in zip(got, want)) and got[2].dtype == np.uint16


def affine_links(k):
    """Grid space -> the space of source k (origin 0): p - offset, with a small shear."""
    M = np.eye(4)
    M[0, 1], M[1, 2], M[2, 0] = TILTS[k]
    M[:3, 3] = [-v for v in OFFSETS[k]]
    return [Link.linear(M)]


def group(dtype, seed=29):
    rng = np.random.default_rng(seed)
    return [extreme_volume(dtype, SRC_SHAPE, rng, huge_floats=False) for _ in range(len(OFFSETS))]


def device(images, grid, interpolation=1, background=0.0, min_count=1, fill=0.0):
    """`images` as cover_restate.restate takes them, through CoverAverage."""
    acc = CoverAverage(grid)
    for links, vol, o, s, mask in images:
        acc.add(vol if links is None else (vol, o, s), None if links is None else Chain(links), mask, interpolation, background)
    out = acc.finish(min_count, fill)
    acc.close()
    return out


def main_images(dtype):
    return [(affine_links(k), v, (0.0, 0.0, 0.0), SRC_S, None) for k, v in enumerate(group(dtype))]


def main_outputs():
    """The main comparison's device results, every type and both modes; also computed in a child with small launches."""
    out = {}
    for dtype in ALL_TYPES:
        for mode in (0, 1):
            m, s, c = device(main_images(dtype), GRID, mode, 3.0)
            out[f"mean_{dtype}_{mode}"], out[f"stdev_{dtype}_{mode}"], out[f"count_{dtype}_{mode}"] = m, s, c
    return out


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dtype", ALL_TYPES)
def test_every_type_equals_the_restatement(dtype, mode):
    images = main_images(dtype)
    want = cover_restate.restate(images, GRID, interpolation=mode, background=3.0)
    assert sorted(np.unique(want[2])) == [0, 1, 2, 3, 4, 5]                 # every count occurs
    got = device(images, GRID, mode, 3.0)
    assert same3(got, want), dtype
    assert (got[0][want[2] == 0] == 0).all() and (got[1][want[2] <= 1] == 0).all()
    assert got[1].max() > 0


MASK_O, MASK_S = (2.0, 1.5, 0.25), (1.5, 1.5, 1.5)


def masks(seed=31):
    """9 x 9 x 9 voxels at spacing 1.5: u8 with zeros and non-zeros, i16 with negative values as non-zero."""
    rng = np.random.default_rng(seed)
    u8 = (rng.integers(0, 3, (9, 9, 9)) * 100).astype(np.uint8)
    i16 = rng.choice(np.array([0, 0, -1, -32768, 7], np.int16), size=(9, 9, 9))
    assert (i16 < 0).any() and (u8 == 0).any() and (i16 == 0).any()
    return (u8, MASK_O, MASK_S), (i16, (3.25, 2.0, 1.0), MASK_S)


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_masks_of_another_geometry(dtype):
    m_u8, m_i16 = masks()
    images = [(l, v, o, s, (m_u8, None, m_i16, m_u8, m_i16)[k]) for k, (l, v, o, s, _) in enumerate(main_images(dtype))]
    plain = cover_restate.restate(main_images(dtype), GRID)
    for mode in (0, 1):
        want = cover_restate.restate(images, GRID, interpolation=mode)
        got = device(images, GRID, mode)
        assert same3(got, want), mode
    assert (want[2] < plain[2]).any() and (want[2] > 0).any() and (want[2] <= plain[2]).all()
    # a float mask is refused
    acc = CoverAverage(GRID)
    l, v, o, s, _ = images[0]
    with pytest.raises(_abi.FrogError) as e:
        acc.add((v, o, s), Chain(l), (m_u8[0].astype(np.float32), MASK_O, MASK_S))
    assert e.value.code == _abi.FROG_E_INVALID
    with pytest.raises(_abi.FrogError) as e:
        acc.finish()                                                        # the refused add did not count
    assert e.value.code == _abi.FROG_E_INVALID


def test_without_a_chain():
    rng = np.random.default_rng(37)
    shape = GRID[0][::-1]
    vols = [extreme_volume(dt, shape, rng, huge_floats=False) for dt in ("int16", "float32", "uint32", "float64")]
    on_grid = [rng.integers(-1, 2, shape).astype(dt) for dt in ("int8", "uint16", "int32", "uint8")]
    for with_mask in (False, True):
        images = [(None, v, None, None, m if with_mask else None) for v, m in zip(vols, on_grid)]
        want = cover_restate.restate(images, GRID)
        got = device(images, GRID)
        assert same3(got, want), with_mask
        assert (want[2] == 4).all() != with_mask
    assert same3(cover_average(vols, masks=on_grid), want)
    acc = CoverAverage(GRID)
    for bad in (dict(volume=np.zeros((13, 17, 20), np.int16)), dict(volume=vols[0], mask=np.ones((13, 17, 18), np.uint8))):
        with pytest.raises(_abi.FrogError) as e:
            acc.add(**bad)
        assert e.value.code == _abi.FROG_E_INVALID


def nonlinear_chains():
    """random_chain-style lattices forward, their Newton inverses, and a chain collapsed into one field link."""
    from test_gpu_chain import random_chain
    rng = np.random.default_rng(41)
    forward = random_chain(rng, 2, 0.5)
    inverse = invert(random_chain(rng, 2, 0.5))
    disp, _ = Chain(random_chain(rng, 1, 0.5)).sample((0.0, 0.0, 0.0), (6.0, 6.0, 6.0), (16, 15, 14), determinant=False)
    field = [Link.field((16, 15, 14), (0.0, 0.0, 0.0), (6.0, 6.0, 6.0), disp)]
    return forward, inverse, field, inverse


def test_through_nonlinear_chains():
    """Expected: Chain.reslice of the source, of the ones-volume (inside) and of the mask, composed by the NumPy update."""
    rng = np.random.default_rng(43)
    grid = ((19, 17, 13), (6.0, 9.0, 4.0), (4.0, 4.0, 4.0))
    m_u8, m_i16 = masks()
    images = []
    for k, links in enumerate(nonlinear_chains()):
        vol = rng.uniform(-2000, 2000, SRC_SHAPE).astype(("int16", "float32")[k % 2])
        mask = (None, (m_u8[0], (20.0, 18.0, 10.0), (5.0, 5.0, 5.0)), (m_i16[0], (12.0, 14.0, 8.0), (6.0, 6.0, 6.0)), None)[k]
        images.append((Chain(links), vol, (8.0 + 7.0 * k, 12.0 + 3.5 * k, 6.0 + 2.0 * k), (4.0, 4.5, 3.5), mask))
    for mode in (0, 1):
        want = cover_restate.restate(images, grid, interpolation=mode, reslicer=lambda c, *a: c.reslice(*a))
        acc = CoverAverage(grid)
        for c, vol, o, s, mask in images:
            acc.add((vol, o, s), c, mask, mode)
        got = acc.finish()
        assert np.array_equal(got[2], want[2])
        assert same3(got, want), mode
    assert len(np.unique(want[2])) >= 4 and want[2].max() == 4


def test_exclusive_regions_hold_their_own_image():
    """Two images of 8 x 6 x 5 voxels on a 14 x 6 x 5 grid, the second 4 voxels further along x: x < 4 is the first image's
    alone, 4 <= x < 8 both, 8 <= x < 12 the second's alone, x >= 12 nobody's."""
    rng = np.random.default_rng(47)
    grid = ((14, 6, 5), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    a = rng.integers(100, 3000, (5, 6, 8)).astype(np.int16)
    b = rng.integers(100, 3000, (5, 6, 8)).astype(np.int16)
    vols = [(a, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), (b, (4.0, 0.0, 0.0), (1.0, 1.0, 1.0))]
    chains = [Chain([]), Chain([])]
    mean, stdev, count = cover_average(vols, chains, grid=grid)
    assert (count[:, :, :4] == 1).all() and (count[:, :, 4:8] == 2).all() and (count[:, :, 8:12] == 1).all() and (count[:, :, 12:] == 0).all()
    assert same(mean[:, :, :4], a[:, :, :4].astype(np.float32)) and same(mean[:, :, 8:12], b[:, :, 4:].astype(np.float32))
    assert (stdev[:, :, :4] == 0).all() and (stdev[:, :, 8:] == 0).all() and (mean[:, :, 12:] == 0).all()
    fa, fb = a[:, :, 4:].astype(np.float32), b[:, :, :4].astype(np.float32)
    assert same(mean[:, :, 4:8], fa + (fb - fa) / np.float32(2))
    plain, _ = average(vols, chains, grid, 1, -1024.0)
    assert (plain[:, :, :4] != mean[:, :, :4]).all() and (plain[:, :, 8:12] != mean[:, :, 8:12]).all()      # dimmed by the background
    assert same(plain[:, :, 4:8], fa / np.float32(2) + fb / np.float32(2))
    m2, s2, c2 = cover_average(vols, chains, grid=grid, min_count=2, fill=-1024.0)
    assert same(c2, count) and same(m2[:, :, 4:8], mean[:, :, 4:8]) and same(s2[:, :, 4:8], stdev[:, :, 4:8])
    for region in (np.s_[:, :, :4], np.s_[:, :, 8:]):
        assert (m2[region] == -1024.0).all() and (s2[region] == 0).all()
    with pytest.raises(_abi.FrogError) as e:
        cover_average(vols, chains, grid=grid, min_count=0)
    assert e.value.code == _abi.FROG_E_INVALID


def test_resliced_output_and_later_finishes():
    images = main_images("int16")
    acc = CoverAverage(GRID)
    with pytest.raises(_abi.FrogError) as e:
        acc.finish()                                                        # before the first add
    assert e.value.code == _abi.FROG_E_INVALID
    state = cover_restate.start(GRID[0][::-1])
    for k, (links, vol, o, s, _) in enumerate(images):
        c = Chain(links)
        r = acc.add((vol, o, s), c, None, k % 2, -700.0, resliced=True)
        assert same(r, c.reslice(vol, o, s, *GRID, k % 2, -700.0))
        assert (r == -700).any()                                            # the background shows in the resliced volume only
        x, valid, _ = cover_restate.terms(links, vol, o, s, GRID, None, k % 2, -700.0)
        state = cover_restate.update(state, x, valid)
        if k == 2:
            first = acc.finish()
            again = acc.finish()
            assert same3(first, again) and same3(first, cover_restate.finish(state))
    assert same3(acc.finish(), cover_restate.finish(state))                 # the adds after a finish continued the sequence
    assert same3(acc.finish(3, 9.5), cover_restate.finish(state, 3, 9.5))
    # any output alone
    lib, n = acc._lib, int(np.prod(GRID[0]))
    mean, count = np.empty(n, np.float32), np.empty(n, np.uint16)
    assert lib.frog_cover_finish(acc._h, 1, 0.0, mean.ctypes.data_as(_abi.c_float_p), None, None) == 0
    assert lib.frog_cover_finish(acc._h, 1, 0.0, None, None, count.ctypes.data_as(_abi.C.POINTER(_abi.C.c_uint16))) == 0
    want = cover_restate.finish(state)
    assert same(mean, want[0].ravel()) and same(count, want[2].ravel())
    assert lib.frog_cover_finish(acc._h, 1, 0.0, None, None, None) == _abi.FROG_E_INVALID


def test_small_launch_chunks_give_the_same_bytes(tmp_path):
    """FROG_CHAIN_LAUNCH_MAX=512 (read once per process: a child): nine launches per kernel over the grid."""
    path = str(tmp_path / "chunks.npz")
    code = "import sys; sys.path[:0] = [%r, %r]; import numpy as np, test_gpu_cover as t; np.savez(%r, **t.main_outputs())" % (ROOT, HERE, path)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, FROG_CHAIN_LAUNCH_MAX="512"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    chunked = dict(np.load(path))
    plain = main_outputs()
    assert sorted(chunked) == sorted(plain) and len(plain) == 48
    for k, v in plain.items():
        assert v.dtype == chunked[k].dtype and v.tobytes() == chunked[k].tobytes(), k


def run(args, cwd, timeout=300):
    return subprocess.run(args, cwd=cwd, capture_output=True, text=True, timeout=timeout)


def test_average_image_coverage_end_to_end(tmp_path):
    from test_chain import smooth_chain
    from test_gpu_chain import _write_chain
    d = tmp_path
    rng = np.random.default_rng(53)
    (d / "bbox.json").write_text(json.dumps({"bbox": [[0.0, 0.0, 0.0], [60.0, 52.0, 44.0]]}))
    (d / "transforms").mkdir()
    names, mask_names = [], []
    z, y, x = np.meshgrid(np.arange(14), np.arange(16), np.arange(18), indexing="ij")
    for i, dt in enumerate(("int16", "float32", "uint8")):
        _write_chain(d / "transforms" / f"{i}.json", smooth_chain(seed=60 + i, amplitude=1.0))
        v = (100 + 60 * np.sin(x / (3.0 + i)) * np.cos(y / 4.0) + 5 * z + rng.normal(0, 2, x.shape)).astype(dt)
        names.append(f"v{i}.nii.gz")
        write_volume(d / names[-1], v, (2.0 + 9.0 * i, 1.0 + 5.0 * i, 3.0 * i), (2.5, 2.5, 3.0))
        m = (rng.integers(0, 4, (8, 8, 8)) - 1).astype(("uint8", "int16", "int8")[i]) if i != 1 else rng.integers(-2, 2, (8, 8, 8)).astype(np.int16)
        mask_names.append(f"m{i}.nii.gz")
        write_volume(d / mask_names[-1], m, (4.0 + 8.0 * i, 2.0 + 6.0 * i, 1.0 + 2.0 * i), (5.0, 5.0, 5.0))
    (d / "masks.txt").write_text("\n".join(mask_names) + "\n")
    spacing = "4"
    r = run([os.path.join(BIN, "DummyVolumeGenerator"), "bbox.json", spacing], d)
    assert r.returncode == 0, r.stdout + r.stderr
    for i, v in enumerate(names):
        r = run([os.path.join(BIN, "VolumeTransform"), v, "dummy.mhd", "-t", f"transforms/{i}.json", "-o", f"flow_{i}.nii.gz"], d)
        assert r.returncode == 0, r.stdout + r.stderr
    r = run([os.path.join(BIN, "AverageImage"), "bbox.json", spacing] + names + ["-o", "cov", "-c", "1", "-ml", "masks.txt", "-wt", "1",
                                                                                  "-mc", "2", "-f", "-5"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    grid = bbox_grid(d / "bbox.json", float(spacing))
    vols = [read_volume(d / n) for n in names]
    mask_vols = [read_volume(d / n) for n in mask_names]
    chains = [Chain(invert(read_transform(d / "transforms" / f"{i}.json"))) for i in range(3)]
    want = cover_average(vols, chains, mask_vols, grid, min_count=2, fill=-5.0)
    assert want[2].min() == 0 and want[2].max() >= 2 and (want[0] == -5).any() and (want[1] > 0).any()
    for name, w in zip(("average.nii.gz", "stdev.nii.gz", "coverage.nii.gz"), want):
        got, o, s = read_volume(d / "cov" / name)
        assert same(got, w) and o == grid[1] and s == grid[2], name
    for i in range(3):
        a, oa, sa = read_volume(d / f"flow_{i}.nii.gz")
        b, ob, sb = read_volume(d / "cov" / f"transformed{i}.nii.gz")
        assert same(a, b) and oa == ob and sa == sb, i
    # without -c: the plain average as before, and no coverage file
    r = run([os.path.join(BIN, "AverageImage"), "bbox.json", spacing] + names + ["-o", "plain", "-wt", "1"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    pm, ps = average(vols, chains, grid)
    for name, w in (("average.nii.gz", pm), ("stdev.nii.gz", ps)):
        got, _, _ = read_volume(d / "plain" / name)
        assert same(got, w), name
    assert not (d / "plain" / "coverage.nii.gz").exists()
    for i in range(3):
        assert same(read_volume(d / "plain" / f"transformed{i}.nii.gz")[0], read_volume(d / f"flow_{i}.nii.gz")[0])
    # a float mask is named before anything is written
    write_volume(d / "mf.nii.gz", mask_vols[0][0].astype(np.float32), mask_vols[0][1], mask_vols[0][2])
    (d / "bad.txt").write_text("mf.nii.gz\nm1.nii.gz\nm2.nii.gz\n")
    r = run([os.path.join(BIN, "AverageImage"), "bbox.json", spacing] + names + ["-o", "bad", "-c", "1", "-ml", "bad.txt"], d)
    assert r.returncode == 1 and "mf.nii.gz" in r.stdout and not (d / "bad").exists()
