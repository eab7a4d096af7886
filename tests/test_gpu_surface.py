"""The distance transform and the surface distances on the device (frog_distance_map, frog_surface, include/frog_chain.h;
frog_amd.volume.distance_map / SurfaceDistances / surface_distances; bin/FuseLabels -d 1) against their NumPy restatement
(surface_restate.py).  Distances are fixed point and everything built on them is integer arithmetic: every comparison is ==."""
import csv
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from frog_amd import _abi
from frog_amd.chain import Chain, Link, invert, read_transform
from frog_amd.volume import (SURFACE_ROW, SurfaceDistances, bbox_grid, distance_map, read_volume, robust_z, surface_distances,
                             surface_metrics, write_volume)

import labels_restate
import surface_restate as sr
from test_gpu_labels import POOL, TYPES, _label_volumes, run

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")
DIMS = (19, 13, 7)                                          # 1729 voxels: seven blocks of 256, the last one partial
SHAPE = DIMS[::-1]
SPACINGS = [(1.0, 1.0, 1.0), (0.5, 2.0, 1.25), (0.7, 1.3, 2.1)]
VALUES = [-3, 58, 86, 170, 1247, 29193, 40358]             # POOL without the background


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def same_rows(got, want):
    return got.shape == want.shape and all(np.array_equal(got[k], want[k]) and got[k].dtype == want[k].dtype for k in SURFACE_ROW.names)


def check_map(m, value, spacing):
    for mode in (0, 1):
        got = distance_map(m, value, spacing, mode)
        assert same(got, sr.distance_map(m, value, spacing, mode)), (value, spacing, mode)


# ---- frog_distance_map -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spacing", SPACINGS)
def test_distance_map_of_random_empty_full_and_corner_sets(spacing):
    rng = np.random.default_rng(3)
    for density in (0.02, 0.5):
        check_map(np.where(rng.random(SHAPE) < density, 58, 0).astype(np.uint8), 58, spacing)
    empty = np.zeros(SHAPE, np.uint8)
    check_map(empty, 58, spacing)
    assert (distance_map(empty, 58, spacing) == 0xFFFFFFFF).all()
    check_map(np.full(SHAPE, 58, np.uint8), 58, spacing)
    assert (distance_map(np.full(SHAPE, 58, np.uint8), 58, spacing) == 0).all()
    for z in (0, SHAPE[0] - 1):
        for y in (0, SHAPE[1] - 1):
            for x in (0, SHAPE[2] - 1):
                m = np.zeros(SHAPE, np.uint8)
                m[z, y, x] = 58
                check_map(m, 58, spacing)


@pytest.mark.parametrize("dtype", TYPES)
def test_distance_map_of_every_integer_type(dtype):
    rng = np.random.default_rng(11)
    m = rng.choice(POOL[dtype], size=SHAPE).astype(dtype)
    value = POOL[dtype][-1]                                 # -3 in the int8 map
    assert (m == value).any() and (dtype != "int8" or value == -3)
    check_map(m, value, (0.5, 2.0, 1.25))


@pytest.mark.parametrize("axis", (0, 1, 2))
def test_distance_map_of_lines_longer_than_a_wave_a_block_and_any_tile(axis):
    dims = [(300, 3, 2), (3, 300, 2), (2, 3, 300)][axis]
    shape = dims[::-1]
    for ends in ((0,), (0, 299)):
        m = np.zeros(shape, np.int16)
        for e in ends:
            at = [1, 1, 1]
            at[2 - axis] = e                                # [z, y, x]
            at = [min(a, s - 1) for a, s in zip(at, shape)]
            m[tuple(at)] = 1247
        check_map(m, 1247, (0.7, 1.3, 2.1))
        far = distance_map(m, 1247, (1.0, 1.0, 1.0), 0)
        assert far.max() >= (149 if len(ends) == 2 else 299) * 65536


# ---- frog_surface ------------------------------------------------------------------------------------------------------------

def box(x0, x1, y0=3, y1=9, z0=2, z1=5, value=58, dtype=np.uint8):
    m = np.zeros(SHAPE, dtype)
    m[z0:z1, y0:y1, x0:x1] = value
    return m


def device_rows(images, reference, values, spacing, percentile=95, **kw):
    with SurfaceDistances(reference, values, spacing, percentile) as acc:
        return [acc.add(m, **kw) for m in images]


def test_designed_cases():
    reference, image = box(4, 10), box(6, 12)
    got, = device_rows([image], reference, [58], (1.5, 1.0, 1.0))
    assert same_rows(got, sr.rows(image, reference, [58], (1.5, 1.0, 1.0)).astype(SURFACE_ROW))
    assert surface_metrics(got)[0][0] == 3.0
    got, = device_rows([reference], reference, [58], (0.7, 1.3, 2.1))
    assert got["n_a"][0] == got["n_b"][0] > 0 and all(got[k][0] == 0 for k in SURFACE_ROW.names[2:])
    a, b = np.zeros(SHAPE, np.int16), np.zeros(SHAPE, np.int16)
    a[1, 2, 3] = -3
    b[4, 6, 6] = -3
    got, = device_rows([a], b, [-3], (1.0, 1.0, 1.0))
    assert same_rows(got, sr.rows(a, b, [-3], (1.0, 1.0, 1.0)).astype(SURFACE_ROW))
    assert got["max_ab"][0] == int(np.rint(np.sqrt(34.0) * 65536)) and got["n_a"][0] == 1
    full, flush = np.full(SHAPE, 58, np.uint8), box(0, 5)   # surface on the grid's border
    got, = device_rows([flush], full, [58], (1.0, 1.0, 1.0))
    want = sr.rows(flush, full, [58], (1.0, 1.0, 1.0)).astype(SURFACE_ROW)
    assert same_rows(got, want) and got["n_b"][0] == 1729 - 17 * 11 * 5 and got["n_a"][0] == 90 - 3 * 4 * 1


def test_absent_labels_and_labels_that_are_not_measured():
    reference = box(4, 10)
    reference[0, :, :] = 86                                 # 86: in the reference, absent from the image
    image = box(5, 11)
    image[6, :, :] = 170                                    # 170: in the image, absent from the reference
    image[3, 5:7, 6:9] = 99                                 # 99 is not measured; it makes surface inside the 58 box
    values = [58, 86, 170]
    got, = device_rows([image], reference, values, (0.5, 2.0, 1.25))
    want = sr.rows(image, reference, values, (0.5, 2.0, 1.25)).astype(SURFACE_ROW)
    assert same_rows(got, want)
    assert (got["n_a"][1], got["n_b"][2]) == (0, 0) and got["n_b"][1] > 0 and got["n_a"][2] > 0
    for l in (1, 2):
        assert got["sum_ab"][l] == got["sum_ba"][l] == 0 and all(got[k][l] == 0xFFFFFFFF for k in SURFACE_ROW.names[4:])
    assert all(np.isnan(m[1:]).all() and np.isfinite(m[0]) for m in surface_metrics(got))
    plain = image.copy()
    plain[plain == 99] = 58
    assert got["n_a"][0] > sr.rows(plain, reference, [58], (0.5, 2.0, 1.25))["n_a"][0]


def radlex_group():
    """Six label maps on the grid, one per integer type: blocks of the RadLex-like POOL's values (narrowed per type), each
    image shifted and with a tenth of its voxels redrawn; the reference is the int32 image of the same blocks, unshifted."""
    rng = np.random.default_rng(29)
    z, y, x = np.indices(SHAPE)
    block = (x // 5) + 3 * (y // 6) + 7 * (z // 4)
    pool = np.array(POOL["int32"])
    reference = pool[block % len(pool)].astype(np.int32)
    images = []
    for k, dt in enumerate(TYPES):
        own = np.array(POOL[dt])
        m = np.roll(own[block % len(own)], (k % 2, k % 3, k), (0, 1, 2))
        noise = rng.random(SHAPE) < 0.1
        m[noise] = rng.choice(own, size=int(noise.sum()))
        images.append(m.astype(dt))
    return images, reference


@pytest.mark.parametrize("percentile", (1, 50, 95, 100))
def test_a_group_of_every_type_and_the_percentiles(percentile):
    images, reference = radlex_group()
    spacing = (0.7, 1.3, 2.1)
    got = device_rows(images + images[:1], reference, VALUES, spacing, percentile)
    for m, rows in zip(images, got):
        assert same_rows(rows, sr.rows(m, reference, VALUES, spacing, percentile).astype(SURFACE_ROW)), m.dtype
    assert same_rows(got[-1], got[0])                       # no state leaks from one add into the next
    assert got[1]["n_a"][0] > 0 and got[0]["n_a"][0] == 0   # -3 lives in the int8 image alone
    again = device_rows(images, reference, VALUES, spacing, percentile)
    assert all(same_rows(a, b) for a, b in zip(again, got))


def dump(path):
    """The child of test_launch_splitting: the group's rows and one distance map into an .npz."""
    images, reference = radlex_group()
    rows = device_rows(images, reference, VALUES, (0.7, 1.3, 2.1))
    np.savez(path, rows=np.stack(rows), map0=distance_map(reference, 58, (0.7, 1.3, 2.1), 0), map1=distance_map(reference, 58, (0.7, 1.3, 2.1), 1))


def test_launch_splitting(tmp_path):
    """FROG_CHAIN_LAUNCH_MAX=256: seven launches per kernel over the grid, four lines per launch of the x pass."""
    path = str(tmp_path / "split.npz")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_surface as t; t.dump(%r)" % (ROOT, os.path.join(ROOT, "tests"), path)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, FROG_CHAIN_LAUNCH_MAX="256"), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.load(path)
    images, reference = radlex_group()
    want = np.stack(device_rows(images, reference, VALUES, (0.7, 1.3, 2.1)))
    assert same_rows(got["rows"], want)
    assert same(got["map0"], sr.distance_map(reference, 58, (0.7, 1.3, 2.1), 0))
    assert same(got["map1"], sr.distance_map(reference, 58, (0.7, 1.3, 2.1), 1))


# ---- through a chain ---------------------------------------------------------------------------------------------------------

def translation(voxels, spacing):
    m = np.eye(4)
    m[:3, 3] = [v * s for v, s in zip(voxels, spacing)]
    return Chain([Link.linear(m)])


def test_a_whole_voxel_translation_gives_the_rows_of_the_shifted_volume():
    spacing = (0.5, 2.0, 1.25)
    grid = (DIMS, (0.0, 0.0, 0.0), spacing)
    images, reference = radlex_group()
    image = images[3]
    chain = translation((2, -1, 1), spacing)                # grid voxel (x, y, z) reads source voxel (x + 2, y - 1, z + 1)
    shifted = chain.reslice(image, (0.0, 0.0, 0.0), spacing, DIMS, (0.0, 0.0, 0.0), spacing, 0, 170.0)
    want = np.full(SHAPE, 170, image.dtype)
    want[:-1, 1:, :-2] = image[1:, :-1, 2:]
    assert same(shifted, want)
    with SurfaceDistances(reference, VALUES, grid) as acc:
        through = acc.add((image, (0.0, 0.0, 0.0), spacing), chain, 170.0)
        direct = acc.add(shifted)
    assert same_rows(through, direct)
    assert same_rows(direct, sr.rows(shifted, reference, VALUES, spacing).astype(SURFACE_ROW))


def test_the_label_at_every_voxel_is_the_reslice_s():
    """A one-voxel-thick sheet is all surface: n_a and the distances are those of exactly the voxels frog_chain_reslice
    labels, through a chain that is no whole-voxel shift and a source with its own geometry."""
    spacing = (1.0, 1.0, 1.0)
    grid = (DIMS, (0.0, 0.0, 0.0), spacing)
    source = np.zeros((9, 15, 23), np.uint16)
    source[4, :, :] = 1247                                  # a sheet
    source[:, 7, 3:20] = 1247                               # crossed by another
    geometry = ((-1.3, -0.8, -0.6), (0.9, 0.95, 0.85))
    m = np.eye(4)
    m[:3, :3] = [[0.98, 0.05, 0.0], [-0.05, 0.98, 0.03], [0.0, -0.03, 1.01]]
    m[:3, 3] = [0.4, -0.3, 0.2]
    chain = Chain([Link.linear(m)])
    resliced = chain.reslice(source, geometry[0], geometry[1], DIMS, (0.0, 0.0, 0.0), spacing, 0, 0.0)
    assert 50 < (resliced == 1247).sum() < 1000
    reference = np.zeros(SHAPE, np.uint16)
    reference[3, :, :] = 1247
    with SurfaceDistances(reference, [1247], grid) as acc:
        through = acc.add((source,) + geometry, chain, 0.0)
    assert same_rows(through, sr.rows(resliced, reference, [1247], spacing).astype(SURFACE_ROW))


# ---- what the feature is for -------------------------------------------------------------------------------------------------

def test_a_shifted_image_stands_out_in_millimetres_whatever_the_structure_s_size():
    """Eight images of a large and a small box, one image translated by 3 voxels along every axis.  Both structures move by
    the same vector, every face 3 voxels along its normal, so both surfaces are between 3 voxels and 3 sqrt(3) voxels off
    over most of their area: the two assd lie within a factor of two of each other and above one voxel, while the Dice of the
    small structure, which no longer overlaps itself, drops by more than that of the large one."""
    shape, spacing = (20, 28, 44), (1.5, 1.5, 1.5)
    base = np.zeros(shape, np.uint8)
    base[2:14, 3:21, 4:30] = 58                             # a large structure
    base[6:9, 10:13, 32:35] = 86                            # a small one beside it
    rng = np.random.default_rng(37)
    images = []
    for k in range(8):
        m = base.copy()
        m[sr.surface(base, 58) & (rng.random(shape) < 0.05)] = 0   # a little boundary noise in every image
        images.append(m)
    reference = labels_restate.restate(images)["labels"].astype(np.uint8)
    without = labels_restate.dice(labels_restate.restate(images))
    images[5] = np.roll(images[5], (3, 3, 3), (0, 1, 2))    # nothing wraps: both boxes stay inside the grid
    with_shift = labels_restate.dice(labels_restate.restate(images))
    out = surface_distances(images, reference, [58, 86], grid=(shape[::-1], (0.0, 0.0, 0.0), spacing))
    for k, m in enumerate(images):
        assert same_rows(out["rows"][k], sr.rows(m, reference, [58, 86], spacing).astype(SURFACE_ROW)), k
    assert int(np.argmax(out["mean_assd"])) == 5 and out["mean_assd_robust_z"][5] > 3
    assert (out["hausdorff"][5] >= 3 * 1.5).all()
    drop = without - with_shift                             # values 0, 58, 86
    assert 0 < drop[1] < drop[2]
    assd = out["assd"][5]
    assert (assd > 1.5).all() and 0.5 < assd[0] / assd[1] < 2.0


# ---- the tool ----------------------------------------------------------------------------------------------------------------

def bits(text):
    return struct.pack("<d", float(text))


def read_csv(path):
    with open(path) as fh:
        return list(csv.reader(fh))


def check_surface_csvs(out_dir, want, names, percentile):
    rows = read_csv(out_dir / "surface.csv")
    assert rows[0] == ["image", "file", "label", "surface_voxels", "reference_surface_voxels", "hausdorff", f"hausdorff_{percentile}", "assd"]
    n, values = len(names), want["values"]
    assert len(rows) == 1 + n * len(values)
    for i in range(n):
        for l, value in enumerate(values):
            row = rows[1 + i * len(values) + l]
            assert row[:3] == [str(i), names[i], str(int(value))]
            assert (int(row[3]), int(row[4])) == (want["rows"][i, l]["n_a"], want["rows"][i, l]["n_b"])
            for text, key in zip(row[5:], ("hausdorff", "hausdorff_p", "assd")):
                assert bits(text) == bits(want[key][i, l]), (i, value, key)
    rows = read_csv(out_dir / "surface_images.csv")
    assert rows[0] == ["image", "file", "labels_measured", "mean_assd", "mean_assd_robust_z", "max_hausdorff"] and len(rows) == 1 + n
    for i, row in enumerate(rows[1:]):
        assert row[:3] == [str(i), names[i], str(int(want["labels_measured"][i]))]
        for text, key in zip(row[3:], ("mean_assd", "mean_assd_robust_z", "max_hausdorff")):
            assert bits(text) == bits(want[key][i]), (i, key)
    rows = read_csv(out_dir / "surface_labels.csv")
    assert rows[0] == ["label", "images_measured", "mean_assd", "max_hausdorff", f"mean_hausdorff_{percentile}"] and len(rows) == 1 + len(values)
    for l, row in enumerate(rows[1:]):
        assert row[:2] == [str(int(values[l])), str(int(want["images_measured"][l]))]
        for text, key in zip(row[2:], ("label_mean_assd", "label_max_hausdorff", "label_mean_hausdorff_p")):
            assert bits(text) == bits(want[key][l]), (l, key)


def test_fuse_labels_measures_the_group_against_its_consensus(tmp_path, small_pairs):
    d = tmp_path
    small_pairs.write(d / "pairs.bin")
    r = run([os.path.join(BIN, "frog"), "pairs.bin", "-li", "12", "-dl", "2", "-di", "8", "-q", "1"], d)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    names = _label_volumes(small_pairs, d)
    n, spacing = small_pairs.n_images, "6.5"
    tool = [os.path.join(BIN, "FuseLabels"), "bbox.json", spacing] + names
    r = run(tool + ["-o", "plain", "-s", "1"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    r = run(tool + ["-o", "vote", "-s", "1", "-d", "1"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "surface : " in r.stdout
    r = run(tool + ["-o", "em", "-s", "1", "-d", "1", "-dr", "1", "-dp", "50"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    plain = sorted(p.name for p in (d / "plain").iterdir())
    for out in ("vote", "em"):
        assert sorted(p.name for p in (d / out).iterdir()) == sorted(plain + ["surface.csv", "surface_images.csv", "surface_labels.csv"])
        for name in plain:
            assert (d / out / name).read_bytes() == (d / "plain" / name).read_bytes(), (out, name)

    grid = bbox_grid(d / "bbox.json", float(spacing))
    vols = [read_volume(d / name) for name in names]
    chains = [Chain(invert(read_transform(d / "transforms" / f"{i}.json"))) for i in range(n)]
    for out, consensus, percentile in (("vote", "labels.nii.gz", 95), ("em", "staple.nii.gz", 50)):
        reference, _, _ = read_volume(d / out / consensus)
        values = [int(row[0]) for row in read_csv(d / out / "labels.csv")[1:] if int(row[0]) != 0]      # the table without -b
        want = surface_distances(vols, reference, values, chains, grid, 0.0, percentile)
        assert len(values) > 5 and np.isfinite(want["mean_assd"]).all()
        check_surface_csvs(d / out, want, names, percentile)
        assert np.array_equal(want["mean_assd_robust_z"], robust_z(want["mean_assd"]))

    # the refusals: exit 1 before anything is written
    for extra, word in ((["-dp", "50"], "-d 1"), (["-dr", "0"], "-d 1"), (["-d", "1", "-dr", "1"], "-s 1"), (["-d", "1", "-dp", "0"], "-dp"),
                        (["-d", "1", "-dp", "101"], "-dp"), (["-d", "1", "-dr", "2"], "-dr"), (["-d", "1", "-ml", "300"], "256")):
        r = run(tool + ["-o", "bad"] + extra, d)
        assert r.returncode == 1 and word in r.stdout and not (d / "bad").exists(), (extra, r.stdout)


# ---- the C ABI's refusals ----------------------------------------------------------------------------------------------------

def test_the_c_abi_refuses_with_a_message():
    lib = _abi.hip_lib()
    m = box(4, 10)

    def view(a, spacing=(1.0, 1.0, 1.0)):
        v = _abi.volume_view(a, (0.0, 0.0, 0.0), spacing)
        v.voxels = a
        return v

    def refused(rc):
        assert rc == _abi.FROG_E_INVALID and len(lib.frog_last_error()) > 10

    out = np.empty(SHAPE, np.uint32)
    out_p = out.ctypes.data_as(_abi.c_u32_p)
    refused(lib.frog_distance_map(None, 58, 0, 0, out_p))
    refused(lib.frog_distance_map(C.byref(view(m)), 58, 0, 0, None))
    refused(lib.frog_distance_map(C.byref(view(m)), 58, 2, 0, out_p))
    refused(lib.frog_distance_map(C.byref(view(m.astype(np.float32))), 58, 0, 0, out_p))
    refused(lib.frog_distance_map(C.byref(view(m, (1.0, 0.0, 1.0))), 58, 0, 0, out_p))
    refused(lib.frog_distance_map(C.byref(view(m, (1.0, float("inf"), 1.0))), 58, 0, 0, out_p))
    values = (C.c_int64 * 3)(58, 86, 170)
    h = C.c_void_p()
    refused(lib.frog_surface_create(None, values, 3, 95, 0, C.byref(h)))
    refused(lib.frog_surface_create(C.byref(view(m)), None, 3, 95, 0, C.byref(h)))
    refused(lib.frog_surface_create(C.byref(view(m)), values, 3, 95, 0, None))
    refused(lib.frog_surface_create(C.byref(view(m)), values, 0, 95, 0, C.byref(h)))
    refused(lib.frog_surface_create(C.byref(view(m)), (C.c_int64 * 257)(*range(257)), 257, 95, 0, C.byref(h)))
    refused(lib.frog_surface_create(C.byref(view(m)), (C.c_int64 * 3)(58, 58, 170), 3, 95, 0, C.byref(h)))
    refused(lib.frog_surface_create(C.byref(view(m)), values, 3, 0, 0, C.byref(h)))
    refused(lib.frog_surface_create(C.byref(view(m)), values, 3, 101, 0, C.byref(h)))
    refused(lib.frog_surface_create(C.byref(view(m.astype(np.float64))), values, 3, 95, 0, C.byref(h)))
    refused(lib.frog_surface_create(C.byref(view(m, (1.0, 1.0, float("nan")))), values, 3, 95, 0, C.byref(h)))
    assert not h.value
    assert lib.frog_surface_create(C.byref(view(m)), values, 3, 95, 0, C.byref(h)) == _abi.FROG_OK
    rows = (_abi.FrogSurfaceRow * 3)()
    refused(lib.frog_surface_add(None, None, C.byref(view(m)), 0.0, rows))
    refused(lib.frog_surface_add(h, None, None, 0.0, rows))
    refused(lib.frog_surface_add(h, None, C.byref(view(m)), 0.0, None))
    refused(lib.frog_surface_add(h, None, C.byref(view(m.astype(np.float32))), 0.0, rows))
    refused(lib.frog_surface_add(h, None, C.byref(view(m)), float("nan"), rows))
    refused(lib.frog_surface_add(h, None, C.byref(view(np.zeros((7, 13, 20), np.uint8))), 0.0, rows))
    assert lib.frog_surface_add(h, None, C.byref(view(m)), 0.0, rows) == _abi.FROG_OK      # none of the refusals left a mark
    assert rows[0].n_a == rows[0].n_b > 0 and rows[0].max_ab == 0 and rows[1].max_ab == 0xFFFFFFFF
    lib.frog_surface_destroy(h)
    lib.frog_surface_destroy(None)
