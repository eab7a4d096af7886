"""The robust group atlas on the device (frog_rank, include/frog_chain.h; frog_amd.volume.RankImages and group_median;
bin/AverageImage -c 1 -r 1) against its NumPy restatement (rank_restate.py).  Order statistics are exact: every comparison
is == on bits, floats through an integer view."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from frog_amd import _abi
from frog_amd.chain import Chain, invert, read_transform
from frog_amd.volume import RankImages, bbox_grid, group_median, rank_planes, read_volume, write_volume

import rank_restate
from test_gpu_cover import ALL_TYPES, GRID, SRC_SHAPE, main_images, masks, same
from test_gpu_cover import device as cover_device

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.path.join(ROOT, "bin")

Q7 = (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0)
REG_MAX = 64                                                # the register tier's largest n_images (k_rank.hip.h)


def same3(got, want):
    return all(same(g, w) for g, w in zip(got, want)) and got[2].dtype == np.uint16


def device(images, grid, interpolation=1, background=0.0, min_count=1, fill=0.0, quantiles=(0.5,), window=None, n_images=None):
    """`images` as cover_restate.restate takes them (links may be a Chain), through RankImages."""
    acc = RankImages(grid, n_images or len(images), window)
    for links, vol, o, s, mask in images:
        chain = None if links is None else (links if isinstance(links, Chain) else Chain(links))
        acc.add(vol if links is None else (vol, o, s), chain, mask, interpolation, background)
    out = acc.finish(min_count, fill, quantiles)
    acc.close()
    return out


def special_images(dtype):
    """test_gpu_cover's five-image group; the float sources also hold +-inf, +-0 and NaN."""
    images = main_images(dtype)
    if np.dtype(dtype).kind == "f":
        for k, (_, v, _, _, _) in enumerate(images):
            flat = v.reshape(-1)
            flat[k::23], flat[k + 5::29], flat[k + 7::31], flat[k + 9::37], flat[k + 11::41] = np.inf, -np.inf, 0.0, -0.0, np.nan
    return images


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dtype", ALL_TYPES)
def test_every_type_equals_the_restatement(dtype, mode):
    images = special_images(dtype)
    want = rank_restate.restate(images, GRID, 2, -9.0, Q7, mode, 3.0)
    assert sorted(np.unique(want[2])) == [0, 1, 2, 3, 4, 5]                 # even and odd k, and k < min_count
    got = device(images, GRID, mode, 3.0, 2, -9.0, Q7)
    assert same3(got, want), dtype
    assert (got[0][:, want[2] < 2] == -9.0).all() and (got[1][want[2] < 2] == 0).all() and np.nanmax(got[1]) > 0
    cover_count = cover_device(images, GRID, mode, 3.0)[2]
    if np.dtype(dtype).kind != "f":
        assert same(got[2], cover_count)
    else:
        assert (got[2] <= cover_count).all() and (mode == 0 or (got[2] < cover_count).any())     # minus the valid NaNs


SIZES = (1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 257, 1000)
SMALL = ((7, 5, 3), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
POOL = np.array([-3.5, -0.0, 0.0, 1.0, 2.5, 1e10], np.float32)


def sized_group(n, distinct):
    """n images on the 7 x 5 x 3 grid with integer masks: voxel v of 105 is valid with probability v / 104, so k runs from 0
    to n within the grid; voxel 1 has every image valid and equal."""
    rng = np.random.default_rng(1000 * n + distinct)
    shape = SMALL[0][::-1]
    if distinct:
        vols = rng.permuted(np.tile((np.arange(n, dtype=np.float32) - n // 2) * np.float32(0.75), (105, 1)), axis=1).T.reshape((n,) + shape).copy()
    else:
        vols = POOL[rng.integers(0, len(POOL), (n,) + shape)]
    p = (np.arange(105) / 104.0).reshape(shape)
    on = rng.random((n,) + shape) < p
    on.reshape(n, -1)[:, 1] = True
    vols.reshape(n, -1)[:, 1] = 2.5
    types = (np.uint8, np.int16, np.int32)
    return [(None, vols[i], None, None, (on[i] * (-3 if i % 3 == 1 else 200)).astype(types[i % 3])) for i in range(n)]


@pytest.mark.parametrize("distinct", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_every_sort_size(n, distinct):
    assert REG_MAX in SIZES and REG_MAX + 1 in SIZES and REG_MAX - 1 in SIZES       # the tier boundary is in the list
    images = sized_group(n, distinct)
    quantiles = Q7 + (0.3,)
    want = rank_restate.restate(images, SMALL, 1, -1.0, quantiles)
    got = device(images, SMALL, 1, 0.0, 1, -1.0, quantiles)
    assert same3(got, want)
    k = want[2].reshape(-1)
    assert k[0] == 0 and k[1] == n and k[-1] == n and (n < 7 or len(np.unique(k)) > 3)
    assert (got[0].reshape(len(quantiles), -1)[:, 1] == 2.5).all() and got[1].reshape(-1)[1] == 0
    assert (got[0].reshape(len(quantiles), -1)[:, 0] == -1.0).all()


def nonlinear_images():
    from test_gpu_chain import random_chain
    rng = np.random.default_rng(71)
    m_u8, m_i16 = masks()
    images = []
    for k in range(5):
        links = random_chain(rng, 1 + k % 2, 0.5)
        vol = rng.uniform(-2000, 2000, SRC_SHAPE).astype(("int16", "float32")[k % 2])
        mask = (None, (m_u8[0], (20.0, 18.0, 10.0), (5.0, 5.0, 5.0)), (m_i16[0], (12.0, 14.0, 8.0), (6.0, 6.0, 6.0)), None, None)[k]
        images.append((links, vol, (8.0 + 5.0 * k, 12.0 + 3.5 * k, 6.0 + 2.0 * k), (4.0, 4.5, 3.5), mask))
    return images


NONLINEAR_GRID = ((19, 17, 13), (6.0, 9.0, 4.0), (4.0, 4.0, 4.0))


def window_outputs():
    """The B-spline group whole and in windows of 1, 4 (ragged last: 4 + 4 + 4 + 1) and 5 (5 + 5 + 3) planes."""
    images = nonlinear_images()
    out = {}
    vols = [(v, o, s) for _, v, o, s, _ in images]
    chains = [Chain(l) for l, _, _, _, _ in images]
    mks = [m for _, _, _, _, m in images]
    for planes in (13, 1, 4, 5):
        med, mad, count, qs = group_median(vols, chains, mks, NONLINEAR_GRID, (0.05, 0.95), max_planes=planes)
        out[f"median_{planes}"], out[f"mad_{planes}"], out[f"count_{planes}"] = med, mad, count
        out[f"q05_{planes}"], out[f"q95_{planes}"] = qs[0.05], qs[0.95]
    return out


def test_order_and_windows(tmp_path):
    images = nonlinear_images()
    chained = [(Chain(l), v, o, s, m) for l, v, o, s, m in images]
    want = rank_restate.restate(chained, NONLINEAR_GRID, quantiles=(0.5, 0.05, 0.95), reslicer=lambda c, *a: c.reslice(*a))
    assert len(np.unique(want[2])) >= 4 and want[2].max() == 5
    got = device(chained, NONLINEAR_GRID, quantiles=(0.5, 0.05, 0.95))
    assert same3(got, want)
    assert same3(device(chained[::-1], NONLINEAR_GRID, quantiles=(0.5, 0.05, 0.95)), want)         # the order of the adds
    plain = window_outputs()
    assert rank_planes(NONLINEAR_GRID, 5) == 13
    for planes in (13, 1, 4, 5):
        for name, w in (("median", want[0][0]), ("q05", want[0][1]), ("q95", want[0][2]), ("mad", want[1]), ("count", want[2])):
            assert same(plain[f"{name}_{planes}"], w), (name, planes)
    # one window alone: planes 4 .. 7
    part = device(chained, NONLINEAR_GRID, quantiles=(0.5, 0.05, 0.95), window=(4, 4))
    assert same3(part, (want[0][:, 4:8], want[1][4:8], want[2][4:8]))
    # small launch chunks (FROG_CHAIN_LAUNCH_MAX is read once per process: a child)
    path = str(tmp_path / "chunks.npz")
    code = "import sys; sys.path[:0] = [%r, %r]; import numpy as np, test_gpu_rank as t; np.savez(%r, **t.window_outputs())" % (ROOT, HERE, path)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, FROG_CHAIN_LAUNCH_MAX="512"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    chunked = dict(np.load(path))
    assert sorted(chunked) == sorted(plain) and len(plain) == 20
    for k, v in plain.items():
        assert v.dtype == chunked[k].dtype and v.tobytes() == chunked[k].tobytes(), k


def test_finish_twice_and_after_further_adds():
    images = special_images("float32")
    acc = RankImages(GRID, 5)
    with pytest.raises(_abi.FrogError) as e:
        acc.finish()                                                        # before the first add
    assert e.value.code == _abi.FROG_E_INVALID
    planes = rank_restate.collect(images, GRID)
    for k, (links, vol, o, s, _) in enumerate(images):
        acc.add((vol, o, s), Chain(links))
        if k == 2:
            first, again = acc.finish(quantiles=Q7), acc.finish(quantiles=Q7)
            assert same3(first, again) and same3(first, rank_restate.finish(planes[:3], quantiles=Q7))
    whole = rank_restate.finish(planes, quantiles=Q7)
    assert same3(acc.finish(quantiles=Q7), whole)                           # the adds after a finish continued
    assert same3(acc.finish(3, 9.5, Q7), rank_restate.finish(planes, 3, 9.5, Q7))
    with pytest.raises(_abi.FrogError) as e:
        acc.add((images[0][1], images[0][2], images[0][3]), Chain(images[0][0]))         # the sixth of five
    assert e.value.code == _abi.FROG_E_INVALID
    # n_q == 0 with only the MAD; any single output has the bits it has beside the others
    values, mad, count = acc.finish(quantiles=(), mad=True, count=False)
    assert values.shape[0] == 0 and count is None and same(mad, whole[1])
    assert same(acc.finish(quantiles=(), mad=False)[2], whole[2])
    alone = acc.finish(quantiles=Q7, mad=False, count=False)
    assert alone[1] is None and alone[2] is None and same(alone[0], whole[0])
    # what finish and add refuse on a live accumulator
    lib, n = acc._lib, int(np.prod(GRID[0]))
    buf, q = np.empty(17 * n, np.float32), (C.c_double * 17)(*([0.5] * 17))
    fp = buf.ctypes.data_as(_abi.c_float_p)
    assert lib.frog_rank_finish(acc._h, 0, 0.0, 1, q, fp, None, None) == _abi.FROG_E_INVALID
    assert lib.frog_rank_finish(acc._h, 1, 0.0, 17, q, fp, None, None) == _abi.FROG_E_INVALID
    assert lib.frog_rank_finish(acc._h, 1, 0.0, 0, None, None, None, None) == _abi.FROG_E_INVALID
    assert lib.frog_rank_finish(acc._h, 1, 0.0, 1, None, fp, None, None) == _abi.FROG_E_INVALID
    for bad in (-0.25, 1.5, float("nan")):
        q[1] = bad
        assert lib.frog_rank_finish(acc._h, 1, 0.0, 2, q, fp, None, None) == _abi.FROG_E_INVALID, bad
    acc.close()
    acc = RankImages(GRID, 2)
    links, vol, o, s, _ = images[0]
    m_u8 = masks()[0]
    for bad in (dict(volume=(vol, o, s), chain=Chain(links), mask=(m_u8[0].astype(np.float32), m_u8[1], m_u8[2])),      # a float mask
                dict(volume=(vol, o, (1.0, 0.0, 1.0)), chain=Chain(links)),                                             # bad geometry
                dict(volume=np.zeros((13, 17, 20), np.int16)), dict(volume=np.zeros(GRID[0][::-1], np.int16), mask=np.ones((13, 17, 18), np.uint8))):
        with pytest.raises(_abi.FrogError) as e:
            acc.add(**bad)
        assert e.value.code == _abi.FROG_E_INVALID
    with pytest.raises(_abi.FrogError) as e:
        acc.finish()                                                        # the refused adds did not count
    assert e.value.code == _abi.FROG_E_INVALID
    acc.close()


def run(args, cwd, timeout=300):
    return subprocess.run(args, cwd=cwd, capture_output=True, text=True, timeout=timeout)


def test_average_image_robust_end_to_end(tmp_path):
    from test_chain import smooth_chain
    from test_gpu_chain import _write_chain
    d = tmp_path
    rng = np.random.default_rng(59)
    (d / "bbox.json").write_text(json.dumps({"bbox": [[0.0, 0.0, 0.0], [60.0, 52.0, 44.0]]}))
    (d / "transforms").mkdir()
    names, mask_names = [], []
    z, y, x = np.meshgrid(np.arange(14), np.arange(16), np.arange(18), indexing="ij")
    for i, dt in enumerate(("int16", "float32", "uint8")):
        _write_chain(d / "transforms" / f"{i}.json", smooth_chain(seed=60 + i, amplitude=1.0))
        v = (100 + 60 * np.sin(x / (3.0 + i)) * np.cos(y / 4.0) + 5 * z + rng.normal(0, 2, x.shape)).astype(dt)
        names.append(f"v{i}.nii.gz")
        write_volume(d / names[-1], v, (2.0 + 9.0 * i, 1.0 + 5.0 * i, 3.0 * i), (2.5, 2.5, 3.0))
        m = (rng.integers(0, 4, (8, 8, 8)) - 1).astype(("uint8", "int16", "int8")[i])
        mask_names.append(f"m{i}.nii.gz")
        write_volume(d / mask_names[-1], m, (4.0 + 8.0 * i, 2.0 + 6.0 * i, 1.0 + 2.0 * i), (5.0, 5.0, 5.0))
    (d / "masks.txt").write_text("\n".join(mask_names) + "\n")
    spacing = "4"
    tool = [os.path.join(BIN, "AverageImage"), "bbox.json", spacing] + names
    common = ["-c", "1", "-ml", "masks.txt", "-mc", "2", "-f", "-5"]
    r = run(tool + ["-o", "plain"] + common, d)
    assert r.returncode == 0, r.stdout + r.stderr
    r = run(tool + ["-o", "robust"] + common + ["-r", "1", "-rq", "0.05,0.95"], d)
    assert r.returncode == 0 and "robust : 1 slab" in r.stdout, r.stdout + r.stderr
    r = run(tool + ["-o", "slabs"] + common + ["-r", "1", "-rq", "0.05,0.95", "-rp", "3"], d)
    assert r.returncode == 0 and "robust : 4 slabs of 3 planes" in r.stdout, r.stdout + r.stderr
    grid = bbox_grid(d / "bbox.json", float(spacing))
    assert grid[0][2] == 11
    vols = [read_volume(d / n) for n in names]
    mask_vols = [read_volume(d / n) for n in mask_names]
    chains = [Chain(invert(read_transform(d / "transforms" / f"{i}.json"))) for i in range(3)]
    median, mad, count, qs = group_median(vols, chains, mask_vols, grid, (0.05, 0.95), min_count=2, fill=-5.0)
    assert count.min() == 0 and count.max() >= 2 and (median == -5).any() and (mad > 0).any()
    files = {"median.nii.gz": median, "mad.nii.gz": mad, "quantile_0.05.nii.gz": qs[0.05], "quantile_0.95.nii.gz": qs[0.95]}
    for name, w in files.items():
        got, o, s = read_volume(d / "robust" / name)
        assert same(got, w) and o == grid[1] and s == grid[2], name
        assert (d / "slabs" / name).read_bytes() == (d / "robust" / name).read_bytes(), name
        assert not (d / "plain" / name).exists()
    for name in ("average.nii.gz", "stdev.nii.gz", "coverage.nii.gz"):
        assert (d / "plain" / name).read_bytes() == (d / "robust" / name).read_bytes(), name
    assert same(read_volume(d / "robust" / "coverage.nii.gz")[0], count)    # integer and finite float sources: no NaN to leave out
    # refused before anything is written
    for k, extra in enumerate((["-r", "1"], ["-c", "1", "-r", "1", "-rq", "1.5"], ["-c", "1", "-rq", "0.5"], ["-c", "1", "-rp", "2"])):
        r = run(tool + ["-o", f"bad{k}"] + extra, d)
        assert r.returncode != 0 and not (d / f"bad{k}").exists(), extra
