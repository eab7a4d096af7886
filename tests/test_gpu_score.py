"""frog_cover_score on the device (include/frog_chain.h; frog_amd.volume.CoverAverage.score, group_quality; bin/AverageImage
-c 1 -q 1) against its NumPy restatement (score_restate.py).  The grid is test_gpu_cover.py's 19 x 17 x 13 = 4199 voxels: three
tiles of 2048, the last one partial with a partial last wave; its five sources give every count from 0 to 5.  Counts, the
histogram and the six f64 sums are compared with == (the sums on their bits)."""
import csv
import ctypes as C
import json
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from frog_amd import _abi
from frog_amd.chain import Chain, Link, invert, read_transform
from frog_amd.volume import CoverAverage, bbox_grid, group_quality, read_volume, write_volume

import cover_restate
import score_restate
from test_gpu_cover import ALL_TYPES, GRID, main_images, masks, nonlinear_chains, same3
from volume_restate import extreme_volume

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.path.join(ROOT, "bin")
# (leave_one_out, min_count, bins): both references, min_count 1, 2, 3, bins 2 and 64 and no histogram
SETTINGS = ((True, 1, 64), (False, 1, 2), (True, 3, 2), (False, 2, 64), (True, 2, 0), (False, 3, 0))


def f64_bits(v):
    return struct.pack("<d", float(v))


def equal(got, want):
    """A score of the device (CoverAverage.score) and of the restatement: counts, histogram and the sums' bits."""
    if got["n"] != want["n"] or got["n_nonfinite"] != want["n_nonfinite"]:
        return False
    if (got["histogram"] is None) != (want["histogram"] is None):
        return False
    if want["histogram"] is not None and not (got["histogram"].dtype == np.uint64 and np.array_equal(got["histogram"], want["histogram"])):
        return False
    return all(f64_bits(got[k]) == f64_bits(want[k]) for k in score_restate.SUMS)


class Both:
    """The same images in a CoverAverage and in the restatement's state."""

    def __init__(self, images, grid, interpolation=1, reslicer=cover_restate.reslice, chain_of=Chain):
        self.acc, self.grid, self.mode, self.reslicer = CoverAverage(grid), grid, interpolation, reslicer
        self.state = cover_restate.start(tuple(int(d) for d in grid[0][::-1]))
        self.chain_of = chain_of
        for image in images:
            self.add(image)

    def parts(self, image):
        links, vol, o, s, mask = image
        return cover_restate.terms(links, vol, o, s, self.grid, mask, self.mode, 0.0, self.reslicer)[:2]

    def add(self, image):
        links, vol, o, s, mask = image
        self.acc.add(vol if links is None else (vol, o, s), None if links is None else self.chain_of(links), mask, self.mode)
        self.state = cover_restate.update(self.state, *self.parts(image))

    def range(self, min_count=1):
        return score_restate.value_range(self.state, min_count)

    def score(self, image, leave_one_out, min_count, bins, value_range=None):
        """(device, restatement)"""
        links, vol, o, s, mask = image
        lo, hi = value_range or self.range()
        got = self.acc.score(vol if links is None else (vol, o, s), None if links is None else self.chain_of(links), mask, self.mode,
                             None, min_count, leave_one_out, bins, (lo, hi))
        x, valid = self.parts(image)
        return got, score_restate.score(self.state, x, valid, min_count, leave_one_out, bins, lo, hi)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dtype", ALL_TYPES)
def test_every_type_equals_the_restatement(dtype, mode):
    images = main_images(dtype)
    b = Both(images, GRID, mode)
    count = b.state[2]
    assert sorted(np.unique(count)) == [0, 1, 2, 3, 4, 5]
    for k, (loo, min_count, bins) in enumerate(SETTINGS):
        image = images[k % len(images)]
        got, want = b.score(image, loo, min_count, bins)
        assert equal(got, want), (dtype, mode, loo, min_count, bins, got, want)
        assert 0 < want["n"] < count.size and want["n_nonfinite"] == 0
        x, valid = b.parts(image)
        if loo and min_count == 1:
            alone = valid & (count == 1)                                    # the image's own voxels: no other image to compare with
            assert alone.any() and want["n"] == int((valid & (count >= 2)).sum())
        if not loo and min_count == 1:
            assert want["n"] == int(valid.sum())
        if bins:
            assert int(got["histogram"].sum()) == got["n"] and got["histogram"].shape == (bins, bins)
        m = score_restate.metrics(want, want["histogram"])
        for name, v in m.items():                                           # the host library's metrics on the device's sums
            assert (math.isnan(v) and math.isnan(got[name])) or abs(got[name] - v) <= 64 * 2.0 ** -52 * max(1.0, abs(v)), name
        assert got["covered_fraction"] == got["n"] / count.size
    b.acc.close()


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_masks_of_another_geometry(dtype):
    m_u8, m_i16 = masks()
    images = [(l, v, o, s, (m_u8, None, m_i16, m_u8, m_i16)[k]) for k, (l, v, o, s, _) in enumerate(main_images(dtype))]
    for mode in (0, 1):
        b = Both(images, GRID, mode)
        for k, image in enumerate(images):
            loo, min_count, bins = SETTINGS[k]
            got, want = b.score(image, loo, min_count, bins)
            assert equal(got, want), (mode, k)
        # a masked image scores on fewer voxels than the same image unmasked, against the same accumulator
        got, want = b.score(images[0], False, 1, 64)
        bare, bare_want = b.score(main_images(dtype)[0], False, 1, 64)
        assert equal(got, want) and equal(bare, bare_want) and 0 < got["n"] < bare["n"]
        b.acc.close()


def test_without_a_chain():
    rng = np.random.default_rng(37)
    shape = GRID[0][::-1]
    vols = [extreme_volume(dt, shape, rng, huge_floats=False) for dt in ("int16", "float32", "uint32", "float64")]
    on_grid = [rng.integers(-1, 2, shape).astype(dt) for dt in ("int8", "uint16", "int32", "uint8")]
    for with_mask in (False, True):
        images = [(None, v, None, None, m if with_mask else None) for v, m in zip(vols, on_grid)]
        b = Both(images, GRID)
        for k, image in enumerate(images):
            for loo, min_count, bins in SETTINGS[k::2]:
                got, want = b.score(image, loo, min_count, bins)
                assert equal(got, want), (with_mask, k, loo, min_count, bins)
        assert with_mask or b.score(images[0], True, 1, 0)[0]["n"] == 4199      # every voxel, four images everywhere
        b.acc.close()


def test_through_nonlinear_chains():
    """Lattices forward, Newton inverses and a field link: value, inside flag and mask from Chain.reslice, as in test_gpu_cover.py."""
    from test_gpu_cover import SRC_SHAPE
    rng = np.random.default_rng(43)
    grid = ((19, 17, 13), (6.0, 9.0, 4.0), (4.0, 4.0, 4.0))
    m_u8, m_i16 = masks()
    images = []
    for k, links in enumerate(nonlinear_chains()):
        vol = rng.uniform(-2000, 2000, SRC_SHAPE).astype(("int16", "float32")[k % 2])
        mask = (None, (m_u8[0], (20.0, 18.0, 10.0), (5.0, 5.0, 5.0)), (m_i16[0], (12.0, 14.0, 8.0), (6.0, 6.0, 6.0)), None)[k]
        images.append((Chain(links), vol, (8.0 + 7.0 * k, 12.0 + 3.5 * k, 6.0 + 2.0 * k), (4.0, 4.5, 3.5), mask))
    for mode in (0, 1):
        b = Both(images, grid, mode, reslicer=lambda c, *a: c.reslice(*a), chain_of=lambda c: c)
        for k, image in enumerate(images):
            for loo, min_count, bins in ((True, 1, 64), (False, 2, 2)):
                got, want = b.score(image, loo, min_count, bins)
                assert equal(got, want), (mode, k, loo)
                assert want["n"] > 0
        b.acc.close()


def test_values_that_are_not_finite():
    """An f32 source with NaN and +-inf: the image itself has x not finite there, and once it is added the mean is not finite
    there either, so every other image meets a y that is not finite."""
    images = main_images("float32")
    rng = np.random.default_rng(59)
    bad = images[1][1].copy()
    flat = bad.ravel()
    flat[rng.choice(flat.size, 40, replace=False)] = np.tile(np.array([np.nan, np.inf, -np.inf, np.nan], np.float32), 10)
    images[1] = (images[1][0], bad) + images[1][2:]
    for mode in (0, 1):
        b = Both(images, GRID, mode)
        lo, hi = -3000.0, 3000.0                                            # the mean's own range is not finite here
        seen = 0
        for k in (1, 0, 2):
            for loo in (True, False):
                got, want = b.score(images[k], loo, 1, 64, (lo, hi))
                assert equal(got, want), (mode, k, loo, got, want)
                assert int(got["histogram"].sum()) == got["n"]
                seen += want["n_nonfinite"]
        assert seen > 0 and b.score(images[1], False, 1, 64, (lo, hi))[1]["n_nonfinite"] > 0
        b.acc.close()


def test_scoring_leaves_the_accumulator_alone():
    images = main_images("int16")
    b = Both(images[:3], GRID)
    before = b.acc.finish()
    first = b.score(images[0], True, 1, 64)
    assert equal(*first)
    assert same3(b.acc.finish(), before) and same3(before, cover_restate.finish(b.state))
    again = b.score(images[0], True, 1, 64)
    assert equal(first[0], again[0]) and np.array_equal(first[0]["histogram"], again[0]["histogram"])      # run to run
    for image in images[3:]:                                                # adds after a score continue the sequence
        b.add(image)
        assert equal(*b.score(image, True, 2, 2))
    assert same3(b.acc.finish(), cover_restate.finish(b.state))
    assert same3(b.acc.finish(3, 9.5), cover_restate.finish(b.state, 3, 9.5))
    # the default range of the Python API is the restatement's
    assert b.acc.quality_range(2) == score_restate.value_range(b.state, 2)
    got = b.acc.score((images[0][1],) + images[0][2:4], Chain(images[0][0]), min_count=2)
    lo, hi = score_restate.value_range(b.state, 2)
    assert equal(got, score_restate.score(b.state, *b.parts(images[0]), 2, True, 64, lo, hi))
    b.acc.close()


def main_outputs():
    """Scores of the main group as arrays; also computed in a child with small launches."""
    out = {}
    for dtype in ("int16", "float32"):
        for mode in (0, 1):
            images = main_images(dtype)
            b = Both(images, GRID, mode)
            for k, (loo, min_count, bins) in enumerate(SETTINGS):
                links, vol, o, s, mask = images[k % len(images)]
                got = b.acc.score((vol, o, s), Chain(links), mask, mode, None, min_count, loo, bins, (-40000.0, 40000.0))
                key = f"{dtype}_{mode}_{k}"
                out["sums_" + key] = np.array([got[name] for name in score_restate.SUMS], np.float64)
                out["n_" + key] = np.array([got["n"], got["n_nonfinite"]], np.uint64)
                if bins:
                    out["hist_" + key] = got["histogram"]
            b.acc.close()
    return out


def test_small_launch_chunks_give_the_same_bytes(tmp_path):
    """FROG_CHAIN_LAUNCH_MAX=512 (read once per process: a child): two tiles per launch, two launches over the three tiles."""
    path = str(tmp_path / "chunks.npz")
    code = "import sys; sys.path[:0] = [%r, %r]; import numpy as np, test_gpu_score as t; np.savez(%r, **t.main_outputs())" % (ROOT, HERE, path)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, FROG_CHAIN_LAUNCH_MAX="512"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    chunked = dict(np.load(path))
    plain = main_outputs()
    assert sorted(chunked) == sorted(plain) and len(plain) == 4 * (6 + 6 + 4)
    for k, v in plain.items():
        assert v.dtype == chunked[k].dtype and v.tobytes() == chunked[k].tobytes(), k


def test_bad_arguments_are_refused():
    lib = _abi.hip_lib()
    images = main_images("int16")
    links, vol, o, s, _ = images[0]
    acc, chain = CoverAverage(GRID), Chain(links)
    src = _abi.volume_view(vol, o, s)
    sums = _abi.FrogScoreSums()
    hist = np.zeros(64 * 64, np.uint64)
    hp = hist.ctypes.data_as(C.POINTER(C.c_uint64))
    INVALID = _abi.FROG_E_INVALID

    def call(a=acc._h, c=chain._h, v=src, mask=None, min_count=1, bins=64, lo=0.0, hi=100.0, out=sums, h=hp):
        return lib.frog_cover_score(a, c, None if v is None else C.byref(v), None if mask is None else C.byref(mask), 1, 0.0, min_count,
                                    1, bins, lo, hi, None if out is None else C.byref(out), h)

    assert call() == INVALID and b"before the first" in lib.frog_last_error()       # no add yet
    acc.add((vol, o, s), chain)
    assert call() == _abi.FROG_OK and sums.n == 0                                   # one image: no other to compare with
    acc.add(images[1][1:4], Chain(images[1][0]))
    assert call() == _abi.FROG_OK and 0 < sums.n < 4199
    assert call(bins=0, h=None) == _abi.FROG_OK
    assert call(a=None) == INVALID and call(v=None) == INVALID and call(out=None) == INVALID
    assert call(min_count=0) == INVALID
    for bins in (1, 65, 1000):
        assert call(bins=bins) == INVALID
    assert call(bins=0) == INVALID and call(h=None) == INVALID                      # bins and the histogram come together
    for lo, hi in ((5.0, 5.0), (7.0, 2.0), (float("nan"), 1.0), (0.0, float("inf")), (float("-inf"), 0.0), (-3e38, 3e38)):
        assert call(lo=lo, hi=hi) == INVALID, (lo, hi)
    # the geometry and mask errors of frog_cover_add
    m_u8 = masks()[0]
    fmask = _abi.volume_view(m_u8[0].astype(np.float32), m_u8[1], m_u8[2])
    assert call(mask=fmask) == INVALID
    nodata = _abi.volume_view(m_u8[0], m_u8[1], m_u8[2]); nodata.data = None
    assert call(mask=nodata) == INVALID
    flat = _abi.volume_view(vol, o, (1.0, 0.0, 1.0))
    assert call(v=flat) == INVALID
    assert call(c=None) == INVALID                                                  # without a chain the dims must be the grid's
    on_grid = _abi.volume_view(np.zeros(GRID[0][::-1], np.int16), GRID[1], GRID[2])
    small = _abi.volume_view(np.ones((13, 17, 18), np.uint8), GRID[1], GRID[2])
    assert call(c=None, v=on_grid) == _abi.FROG_OK and call(c=None, v=on_grid, mask=small) == INVALID
    if lib.frog_device_count() > 1:
        assert call(c=Chain(links, device=1)._h) == INVALID
    acc.close()


def test_group_quality_singles_out_the_displaced_image():
    images, grid = score_restate.ranking_group()
    rows = group_quality([(v, o, s) for _, v, o, s, _ in images], [Chain(l) for l, _, _, _, _ in images], grid=grid)
    want = score_restate.group_quality(images, grid)
    k = score_restate.RANK_DISPLACED
    for name in ("ncc", "nmi"):
        assert min(range(len(rows)), key=lambda i: rows[i][name]) == k, (name, [r[name] for r in rows])
    assert rows[k]["ncc_robust_z"] < -3 and [r["image"] for r in rows] == list(range(6))
    for got, w in zip(rows, want):
        assert equal(got, w)
        assert abs(got["ncc"] - w["ncc"]) <= 2.0 ** -46 and abs(got["nmi"] - w["nmi"]) <= 2.0 ** -46 * 2


def run(args, cwd, timeout=300):
    return subprocess.run(args, cwd=cwd, capture_output=True, text=True, timeout=timeout)


def test_average_image_quality_end_to_end(tmp_path):
    """bin/AverageImage -c 1 -ml ... -q 1 on the ranking group: quality.csv holds the Python API's numbers exactly, and the
    average's three files are those of the run without -q 1, byte for byte."""
    from test_gpu_chain import _write_chain
    d = tmp_path
    images, grid = score_restate.ranking_group()
    (d / "bbox.json").write_text(json.dumps({"bbox": [[0.0, 0.0, 0.0], [19.0, 17.0, 13.0]]}))
    (d / "transforms").mkdir()
    rng = np.random.default_rng(61)
    names, mask_names = [], []
    for i, (links, vol, o, s, _) in enumerate(images):
        _write_chain(d / "transforms" / f"{i}.json", [Link.linear(np.linalg.inv(links[0].matrix))])     # source -> common space
        names.append(f"v{i}.nii.gz")
        write_volume(d / names[-1], vol, o, s)
        mask_names.append(f"m{i}.nii.gz")
        write_volume(d / mask_names[-1], (rng.integers(0, 8, (9, 10, 11)) > 0).astype(np.uint8) * 255, (1.0, 0.5, 0.0), (2.5, 2.5, 2.5))
    (d / "masks.txt").write_text("\n".join(mask_names) + "\n")
    common = [os.path.join(BIN, "AverageImage"), "bbox.json", "1"] + names
    r = run(common + ["-o", "q", "-c", "1", "-ml", "masks.txt", "-mc", "2", "-f", "-5", "-q", "1", "-qb", "32"], d)
    assert r.returncode == 0 and "quality : 32 x 32 bins over [" in r.stdout, r.stdout + r.stderr
    r = run(common + ["-o", "plain", "-c", "1", "-ml", "masks.txt", "-mc", "2", "-f", "-5"], d)
    assert r.returncode == 0 and "quality" not in r.stdout, r.stdout + r.stderr
    for name in ("average.nii.gz", "stdev.nii.gz", "coverage.nii.gz"):
        assert (d / "q" / name).read_bytes() == (d / "plain" / name).read_bytes(), name
    assert not (d / "plain" / "quality.csv").exists()
    g = bbox_grid(d / "bbox.json", 1.0)
    assert g[0] == grid[0]
    vols = [read_volume(d / n) for n in names]
    mask_vols = [read_volume(d / n) for n in mask_names]
    chains = [Chain(invert(read_transform(d / "transforms" / f"{i}.json"))) for i in range(len(names))]
    want = group_quality(vols, chains, mask_vols, g, min_count=2, bins=32)
    with open(d / "q" / "quality.csv", newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == "image,file,voxels,covered_fraction,ncc,nmi,mi,mean_abs_diff,rmse,ncc_robust_z".split(",")
    assert len(rows) == 1 + len(names)
    for i, (row, w) in enumerate(zip(rows[1:], want)):
        assert row[0] == str(i) and row[1] == names[i] and int(row[2]) == w["n"] and 0 < w["n"] < 4199
        for text, name in zip(row[3:], ("covered_fraction", "ncc", "nmi", "mi", "mean_abs_diff", "rmse", "ncc_robust_z")):
            assert f64_bits(float(text)) == f64_bits(w[name]), (i, name, text, w[name])
    k = score_restate.RANK_DISPLACED
    assert min(range(len(want)), key=lambda i: float(rows[1 + i][4])) == k and min(range(len(want)), key=lambda i: float(rows[1 + i][5])) == k
    # an explicit range is used as given
    r = run(common + ["-o", "r", "-c", "1", "-q", "1", "-qb", "8", "-qr", "0", "1500"], d)
    assert r.returncode == 0 and "8 x 8 bins over [0, 1500)" in r.stdout, r.stdout + r.stderr
    want = group_quality(vols, chains, None, g, bins=8, value_range=(0.0, 1500.0))
    with open(d / "r" / "quality.csv", newline="") as f:
        rows = list(csv.reader(f))[1:]
    assert [f64_bits(float(row[5])) for row in rows] == [f64_bits(w["nmi"]) for w in want]
