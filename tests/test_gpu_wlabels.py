"""Locally weighted label fusion on the device (frog_wlabels, include/frog_chain.h; bin/AtlasSegment;
frog_amd.volume.WeightedLabels) against its NumPy restatement (wlabels_restate.py).  The header states every operation and
its order, so every comparison is == on dtype, shape and bits.  The vote kernel's tile is 32 x 8 x 4 voxels: the grids
19 x 13 x 7 (x inside one tile, y and z one tile and a part) and 37 x 11 x 9 (every axis a non-multiple beyond a tile)
put a seam and a partial tile on every axis."""
import csv
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from frog_amd import _abi
from frog_amd.chain import Chain, Link, invert, read_transform
from frog_amd.volume import CoverAverage, Labels, WeightedLabels, atlas_segment, bbox_grid, read_volume, write_volume

import labels_restate
import wlabels_restate
from test_gpu_chain import random_chain
from test_gpu_labels import POOL, TYPES, _label_volumes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")
UNIT = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
GRID_A = ((19, 13, 7),) + UNIT
GRID_B = ((37, 11, 9),) + UNIT
IMAGE_TYPES = ("int16", "uint8", "uint16", "float32", "float64", "float32")


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def mixed_group(grid, seed=29):
    """(target, [(image, labels)] x 6): a float32 target with NaN and inf voxels; images of IMAGE_TYPES that follow the
    target more or less closely (the float ones with NaN, inf and, in float64, values beyond float32); one label type each,
    values from the RadLex-like POOL (-3 in the int8 map, 40358 in the wide ones)."""
    rng = np.random.default_rng(seed)
    shape = grid[0][::-1]
    base = rng.integers(0, 1000, shape).astype(np.float64)
    target = base.astype(np.float32)
    target[1, 2, 3] = np.nan
    target[-1, -1, -1] = np.inf
    target[2, 5, :4] = np.nan
    atlases = []
    for k, (it, lt) in enumerate(zip(IMAGE_TYPES, TYPES)):
        noise = rng.integers(0, 1000, shape)
        mix = (0.1, 0.3, 0.5, 0.7, 0.9, 1.0)[k]
        image = (1 - mix) * base + mix * noise
        if it == "uint8":
            image = image / 4
        if np.dtype(it).kind == "f":
            image = image + 0.25
            image[0, 0, 0] = np.nan
            image[3, 4, 5] = -np.inf
            if it == "float64":
                image[4, 1, 2] = 1e300                          # finite, but not as a float32: no member
                image[4, 1, 3] = -1e-300
        atlases.append((image.astype(it), rng.choice(POOL[lt], size=shape).astype(lt)))
    return target, atlases


def collect(grid, target, atlases, radius, power, floor, fill_label=0, chains=None, target_chain=None, max_labels=0, backgrounds=None):
    """Every output of an accumulator: n_labels, values, the fused map as int32 with its confidence, each alone, the
    probability of every label; with chains the resliced volumes as well."""
    acc = WeightedLabels(grid, len(atlases), max_labels, radius, power, floor)
    bt, bi, bl = backgrounds or (0.0, 0.0, 0.0)
    out = {"resliced_target": acc.target(target, target_chain, 1, bt, resliced=True), "resliced": []}
    for k, (image, labels) in enumerate(atlases):
        out["resliced"].append(acc.add(image, labels, None if chains is None else chains[k], 1, bi, bl, resliced=True))
    out["n_labels"] = acc.finish()
    out["values"] = acc.values()
    out["labels"], out["confidence"] = acc.fused("int32", fill_label)
    out["labels_alone"], out["confidence_alone"] = fused_alone(acc, fill_label)
    out["probability"] = [acc.probability(int(v)) for v in out["values"]]
    out["acc"] = acc
    return out


def fused_alone(acc, fill_label, dtype="int32"):
    labels = np.empty(acc.dims[::-1], np.dtype(dtype))
    confidence = np.empty(acc.dims[::-1], np.float32)
    lv = _abi.volume_view(labels, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    _abi.check(acc._lib.frog_wlabels_fused(acc._h, fill_label, C.byref(lv), None), "frog_wlabels_fused")
    _abi.check(acc._lib.frog_wlabels_fused(acc._h, fill_label, None, confidence.ctypes.data_as(_abi.c_float_p)), "frog_wlabels_fused")
    return labels, confidence


def assert_matches(out, r):
    assert out["n_labels"] == len(r["values"]) and same(out["values"], r["values"])
    assert same(out["labels"], r["labels"].astype(np.int32)) and same(out["labels_alone"], out["labels"])
    assert same(out["confidence"], r["confidence"]) and same(out["confidence_alone"], out["confidence"])
    for l, value in enumerate(r["values"]):
        assert same(out["probability"][l], wlabels_restate.probability(r, value)), value


def invalid(call, *args, **kw):
    with pytest.raises(_abi.FrogError) as e:
        call(*args, **kw)
    assert e.value.code == _abi.FROG_E_INVALID
    return e.value


# ---- 1. every type, radius, power and floor against the restatement -------------------------------------------------------

@pytest.mark.parametrize("grid, radius, power, floor", [
    (GRID_A, 1, 1, 0.0), (GRID_A, 2, 2, 2.0 ** -10), (GRID_B, 3, 8, 2.0 ** -10), (GRID_B, 4, 2, 0.0), (GRID_A, 4, 1, 1.0),
    (GRID_B, 2, 2, 2.0 ** -10), (GRID_B, 1, 8, 0.0), (GRID_A, 3, 2, 1.0)])
def test_types_radii_powers_and_floors(grid, radius, power, floor):
    target, atlases = mixed_group(grid)
    r = wlabels_restate.restate(target, atlases, radius, power, floor, fill_label=-9)
    assert list(r["values"]) == [-3, 0, 58, 86, 170, 1247, 29193, 40358]
    assert (r["total"] == 0).any() and (r["total"] > 0).any()             # the target's NaN voxels have no vote at all
    if floor < 1:
        assert len(np.unique(r["scores"])) > 100                            # the weights do vary
    out = collect(grid, target, atlases, radius, power, floor, fill_label=-9)
    assert_matches(out, r)
    assert (out["labels"][~(r["total"] > 0)] == -9).all()
    assert same(out["resliced_target"], target)                            # without a chain: the source
    for (image, labels), (ri, rl) in zip(atlases, out["resliced"]):
        assert same(ri, image) and same(rl, labels)


# ---- 2. the purpose: one atlas that matches the target outvotes two that do not ---------------------------------------------

def test_a_matching_atlas_outvotes_a_majority_that_does_not():
    rng = np.random.default_rng(5)
    shape = GRID_A[0][::-1]
    t = rng.integers(0, 1000, shape).astype(np.float32)
    images = [(2 * t + 5).astype(np.float32), rng.integers(0, 1000, shape).astype(np.float32), rng.integers(0, 1000, shape).astype(np.float32)]
    maps = [np.full(shape, 1, np.uint8), np.full(shape, 2, np.uint8), np.full(shape, 2, np.uint8)]
    atlases = list(zip(images, maps))
    out = collect(GRID_A, t, atlases, 2, 2, 2.0 ** -10)
    assert (out["labels"] == 1).all()
    majority = Labels(GRID_A, 3)
    for m in maps:
        majority.add(m)
    majority.finish()
    assert (majority.fused()[0] == 2).all()
    r = wlabels_restate.restate(t, atlases, 2, 2, 2.0 ** -10)
    assert (r["scores"][0] == 1.0).all() and r["scores"][1].max() <= 0.32
    assert_matches(out, r)


# ---- 3. floor = 1: the majority vote ------------------------------------------------------------------------------------------

def test_floor_one_is_the_majority_vote_of_frog_labels():
    from test_gpu_labels import vote_group
    maps = vote_group()
    rng = np.random.default_rng(3)
    shape = GRID_A[0][::-1]
    t = rng.integers(0, 1000, shape).astype(np.int16)
    atlases = [(rng.integers(0, 1000, shape).astype(np.int16), m) for m in maps]
    out = collect(GRID_A, t, atlases, 1, 2, 1.0)
    majority = Labels(GRID_A, len(maps))
    for m in maps:
        majority.add(m)
    assert majority.finish() == out["n_labels"]
    values = majority.table()[0]
    labels, agreement = majority.fused("int32")
    assert same(out["values"], values) and same(out["labels"], labels) and same(out["confidence"], agreement)
    for l, v in enumerate(values):
        assert same(out["probability"][l], majority.probability(int(v)))
    assert_matches(out, wlabels_restate.restate(t, atlases, 1, 2, 1.0))


# ---- 4. through chains --------------------------------------------------------------------------------------------------------

def test_through_chains_votes_and_resliced_volumes():
    grid = ((19, 13, 7), (2.0, 3.0, 4.0), (5.0, 7.0, 13.0))
    rng = np.random.default_rng(47)
    chains = [Chain(invert(random_chain(rng, 2, 0.5))) for _ in range(3)]
    off = np.eye(4)
    off[:3, 3] = [38.0, -20.0, 9.0]
    chains.append(Chain([Link.linear(off)]))                                # moves the atlas partly off the grid
    target_chain = Chain(invert(random_chain(rng, 1, 0.5)))
    igeo = ((-3.0, -2.0, -1.0), (3.7, 4.1, 4.6))                           # 28 x 24 x 22 voxels
    lgeo = ((-4.0, -3.0, -2.0), (5.0, 5.9, 6.9))                           # 21 x 17 x 15 voxels
    z, y, x = np.meshgrid(np.arange(22), np.arange(24), np.arange(28), indexing="ij")
    smooth = 300 + 200 * np.sin(x / 3.0) * np.cos(y / 4.0) + 20 * z
    target = ((smooth + rng.normal(0, 10, smooth.shape)).astype(np.float32),) + igeo
    atlases = []
    for k, (it, lt) in enumerate((("int16", "uint8"), ("float32", "int16"), ("uint16", "int32"), ("float64", "uint16"))):
        image = (smooth * (1 + 0.1 * k) + rng.normal(0, 30 * (k + 1), smooth.shape)).astype(it)
        labels = rng.choice(POOL[lt], size=(15, 17, 21)).astype(lt)
        atlases.append(((image,) + igeo, (labels,) + lgeo))
    bt, bi, bl = -7.0, -5.0, 170.0
    out = collect(grid, target, atlases, 2, 2, 2.0 ** -10, chains=chains, target_chain=target_chain, backgrounds=(bt, bi, bl))

    def resliced(volume, chain, interpolation, background):
        a, o, s = volume
        cover = CoverAverage(grid)
        cover.add(volume, chain, None, interpolation, background)
        return chain.reslice(a, o, s, *grid, interpolation, background), cover.finish()[2] == 1

    t, t_inside = resliced(target, target_chain, 1, bt)
    assert same(out["resliced_target"], t) and t_inside.any()
    on_grid = []
    for k, (image, labels) in enumerate(atlases):
        a, inside = resliced(image, chains[k], 1, bi)
        lab, _ = resliced(labels, chains[k], 0, bl)
        assert same(out["resliced"][k][0], a) and same(out["resliced"][k][1], lab), k
        on_grid.append((a, lab, inside))
    assert not on_grid[3][2].all() and on_grid[3][2].any() and (on_grid[3][1] == 170).any()
    r = wlabels_restate.restate(t, on_grid, 2, 2, 2.0 ** -10, target_inside=t_inside)
    assert 170 in r["values"]
    assert_matches(out, r)


# ---- 5. borders -----------------------------------------------------------------------------------------------------------------

def test_borders_constant_target_and_a_slab():
    _, atlases = mixed_group(GRID_B, seed=31)
    atlases = atlases[:3]
    shape = GRID_B[0][::-1]
    flat = np.full(shape, 12, np.int16)
    for floor, power in ((0.25, 3), (0.0, 2)):
        r = wlabels_restate.restate(flat, atlases, 2, power, floor, fill_label=77)
        out = collect(GRID_B, flat, atlases, 2, power, floor, fill_label=77)
        assert_matches(out, r)
        if floor:
            assert set(np.unique(r["scores"])) <= {np.float32(k) * np.float32(floor) ** power for k in range(4)}
        else:
            assert (out["labels"] == 77).all() and (out["confidence"] == 0).all()
            assert all((p == 0).all() for p in out["probability"])
    # patches clipped at all six faces: a perfectly matching atlas keeps the weight 1 up to every corner
    rng = np.random.default_rng(37)
    t = rng.integers(0, 1000, shape).astype(np.float32)
    out = collect(GRID_B, t, [((3 * t + 1).astype(np.float32), np.full(shape, 58, np.uint16))], 3, 2, 0.0)
    assert (out["labels"] == 58).all() and (out["confidence"] == 1).all()
    # a target that is valid on one slab only: votes there and nowhere else, patches one voxel thick
    slab = np.full(shape, np.nan, np.float32)
    slab[4] = t[4]
    r = wlabels_restate.restate(slab, atlases, 1, 1, 0.0, fill_label=-1)
    out = collect(GRID_B, slab, atlases, 1, 1, 0.0, fill_label=-1)
    assert_matches(out, r)
    assert (out["labels"][:4] == -1).all() and (out["labels"][5:] == -1).all() and (out["labels"][4] != -1).any()


# ---- 6. launch splitting and repeatability ----------------------------------------------------------------------------------------

def dump(path):
    """The child of test_launch_splitting: the mixed group's outputs on GRID_B into an .npz."""
    target, atlases = mixed_group(GRID_B)
    out = collect(GRID_B, target, atlases, 2, 2, 2.0 ** -10)
    np.savez(path, values=out["values"], labels=out["labels"], confidence=out["confidence"], probability=np.stack(out["probability"]))


def test_launch_splitting_and_repeatability(tmp_path):
    """FROG_CHAIN_LAUNCH_MAX=512: two blocks per launch -- phase 1 in 512-voxel launches, the vote two tiles at a time (20
    tiles on GRID_B).  The hook is read once per process, hence the child."""
    path = str(tmp_path / "split.npz")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_wlabels as t; t.dump(%r)" % (ROOT, os.path.join(ROOT, "tests"), path)
    env = dict(os.environ, FROG_CHAIN_LAUNCH_MAX="512")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.load(path)
    target, atlases = mixed_group(GRID_B)
    first = collect(GRID_B, target, atlases, 2, 2, 2.0 ** -10)
    second = collect(GRID_B, target, atlases, 2, 2, 2.0 ** -10)
    for out in (second, {k: got[k] for k in got.files}):
        assert same(out["values"], first["values"]) and same(out["labels"], first["labels"]) and same(out["confidence"], first["confidence"])
        assert same(np.stack(list(out["probability"])), np.stack(first["probability"]))


# ---- 7. ties and call order -----------------------------------------------------------------------------------------------------

def test_ties_go_to_the_smaller_value_and_order_is_the_call_order():
    rng = np.random.default_rng(53)
    shape = GRID_A[0][::-1]
    t = rng.integers(0, 1000, shape).astype(np.float32)
    twin = (t + rng.integers(0, 300, shape)).astype(np.float32)
    tie = [(twin, np.full(shape, 86, np.uint8)), (twin, np.full(shape, 58, np.int16))]
    out = collect(GRID_A, t, tie, 2, 2, 0.0)
    assert (out["labels"] == 58).all() and (out["confidence"] == 0.5).all()
    assert_matches(out, wlabels_restate.restate(t, tie, 2, 2, 0.0))
    _, atlases = mixed_group(GRID_A, seed=59)
    atlases = [(image, np.where(labels == 0, 0, 58).astype(labels.dtype)) for image, labels in atlases]      # long sums per plane
    target = mixed_group(GRID_A)[0]
    for order in (atlases, atlases[::-1]):
        assert_matches(collect(GRID_A, target, order, 1, 1, 0.0), wlabels_restate.restate(target, order, 1, 1, 0.0))


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------

def test_protocol_and_refusals():
    grid = ((5, 4, 3),) + UNIT
    rng = np.random.default_rng(43)
    t = rng.integers(0, 100, (3, 4, 5)).astype(np.int16)
    images = [rng.integers(0, 100, (3, 4, 5)).astype(dt) for dt in ("uint8", "float32")]
    maps = [rng.choice([0, 58, 86], size=(3, 4, 5)).astype(dt) for dt in ("uint8", "int16")]
    acc = WeightedLabels(grid, 2, 0, 1, 2, 0.5)
    acc._n_labels = 3
    for getter in (acc.values, lambda: acc.fused("int32"), lambda: acc.probability(0)):
        invalid(getter)                                             # before finish
    invalid(acc.add, images[0], maps[0])                            # before the target
    invalid(acc.target, np.zeros((3, 4, 6), np.int16))              # not on the grid
    acc.target(t)
    invalid(acc.target, t)                                          # a second target
    acc.add(images[0], maps[0])
    invalid(acc.finish)                                             # too few adds
    invalid(acc.add, images[1], maps[1].astype(np.float32))
    invalid(acc.add, images[1], maps[1], None, 1, float("nan"), 0.0)
    invalid(acc.add, images[1], maps[1], None, 1, 0.0, float("inf"))
    invalid(acc.add, np.zeros((3, 4, 6), np.uint8), maps[1])
    invalid(acc.add, images[1], np.zeros((2, 4, 5), np.uint8))
    acc.add(images[1], maps[1])                                     # none of the refused calls counted
    invalid(acc.add, images[0], maps[0])                            # after n_images
    assert acc.finish() == 3
    invalid(acc.add, images[0], maps[0])
    invalid(acc.probability, 57)
    r = wlabels_restate.restate(t, list(zip(images, maps)), 1, 2, 0.5)
    labels, confidence = acc.fused()
    assert labels.dtype == np.uint8 and same(acc.values(), r["values"])
    assert same(labels, r["labels"].astype(np.uint8)) and same(confidence, r["confidence"])
    assert acc.finish() == 3                                        # again: the same answer


def test_a_refused_atlas_leaves_nothing_behind_and_types_that_do_not_fit():
    grid = ((9, 7, 5),) + UNIT                                     # 315 voxels: two blocks
    rng = np.random.default_rng(41)
    shape = grid[0][::-1]
    t = rng.integers(0, 1000, shape).astype(np.float32)
    image = lambda: (t + rng.integers(0, 500, shape)).astype(np.float32)
    good = [(image(), rng.choice(p, size=shape).astype(dt)) for p, dt in (([0, 58], "uint8"), ([0, 58, 86], "int16"), ([0, 58, 86, 1247], "uint16"))]
    bad = [(image(), rng.choice([0, 58, 7, 8, 9], size=shape).astype("uint8")), (image(), rng.choice([1247, 11, 12], size=shape).astype("int32"))]
    acc = WeightedLabels(grid, 3, 4, 1, 2, 2.0 ** -10)
    acc.target(t)
    acc.add(*good[0])
    e = invalid(acc.add, *bad[0])                                  # 0, 58 and three labels of its own: five
    assert "max_labels = 4" in str(e)
    acc.add(*good[1])
    invalid(acc.add, *bad[1])                                      # three known labels and three new ones
    acc.add(*good[2])                                              # the third of n_images = 3: the refused calls did not count
    assert acc.finish() == 4
    r = wlabels_restate.restate(t, good, 1, 2, 2.0 ** -10)
    assert list(acc.values()) == [0, 58, 86, 1247]
    labels, confidence = acc.fused("int32")
    assert same(labels, r["labels"].astype(np.int32)) and same(confidence, r["confidence"])
    for v in r["values"]:
        assert same(acc.probability(int(v)), wlabels_restate.probability(r, v))
    for v in (7, 8, 9, 11, 12):
        invalid(acc.probability, v)
    # 1247 does not fit uint8; a fill label of -1 does not fit uint16, 70000 not int16: nothing is written
    for dtype, fill in (("uint8", 0), ("uint16", -1), ("int16", 70000)):
        labels = np.full(shape, 77, np.dtype(dtype))
        confidence = np.full(shape, -5.0, np.float32)
        lv = _abi.volume_view(labels, *UNIT)
        rc = acc._lib.frog_wlabels_fused(acc._h, fill, C.byref(lv), confidence.ctypes.data_as(_abi.c_float_p))
        assert rc == _abi.FROG_E_INVALID and (labels == 77).all() and (confidence == -5.0).all()
    assert same(acc.fused("uint16", 65535)[0], r["labels"].astype(np.uint16))


# ---- 9. the tool ----------------------------------------------------------------------------------------------------------------

def run(args, cwd, timeout=300):
    return subprocess.run(args, cwd=cwd, capture_output=True, text=True, timeout=timeout)


def test_atlas_segment_matches_the_python_path_and_volume_transform(tmp_path, small_pairs):
    d = tmp_path
    small_pairs.write(d / "pairs.bin")
    r = run([os.path.join(BIN, "frog"), "pairs.bin", "-li", "12", "-dl", "2", "-di", "8", "-q", "1"], d)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    label_names = _label_volumes(small_pairs, d)
    n, spacing = small_pairs.n_images, "6.5"
    rng = np.random.default_rng(61)
    image_names = []
    for i, name in enumerate(label_names):                         # an image on each label map's grid: its blocks, blurred by noise
        lab, o, s = read_volume(d / name)
        image = (lab.astype(np.float64) % 97) * 9 + rng.normal(0, 20, lab.shape)
        image_names.append(f"v{i}.nii.gz")
        write_volume(d / image_names[-1], image.astype(np.int16 if i % 2 else np.float32), o, s)
    lab, o, s = read_volume(d / label_names[0])
    write_volume(d / "target.nii.gz", ((lab.astype(np.float64) % 97) * 9 + rng.normal(0, 20, lab.shape)).astype(np.int16), o, s)
    (d / "labels.txt").write_text("".join(name + "\n" for name in label_names))
    r = run([os.path.join(BIN, "DummyVolumeGenerator"), "bbox.json", spacing], d)
    assert r.returncode == 0, r.stdout + r.stderr
    tool = [os.path.join(BIN, "AtlasSegment"), "bbox.json", spacing, "target.nii.gz"] + image_names + ["-ll", "labels.txt", "-tt", "transforms/0.json"]
    r = run(tool + ["-o", "one", "-wt", "1", "-p", "1", "-f", "-2", "-bl", "86"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "read : " in r.stdout and "device : " in r.stdout and "write : " in r.stdout and "total : " in r.stdout
    one = d / "one"

    # the Python path: the same arrays from Chain objects
    grid = bbox_grid(d / "bbox.json", float(spacing))
    images = [read_volume(d / name) for name in image_names]
    maps = [read_volume(d / name) for name in label_names]
    chains = [Chain(invert(read_transform(d / "transforms" / f"{i}.json"))) for i in range(n)]
    target = read_volume(d / "target.nii.gz")
    want_labels, want_confidence, want_values = atlas_segment(target, images, maps, chains, chains[0], grid, label_background=86.0, fill_label=-2)
    labels, ol, sl = read_volume(one / "segmentation.nii.gz")
    confidence, oc, sc = read_volume(one / "confidence.nii.gz")
    assert ol == oc == tuple(grid[1]) and sl == sc == tuple(grid[2])
    assert want_values[0] == -3 and labels.dtype == np.int16 and same(labels, want_labels) and same(confidence, want_confidence)
    assert len(np.unique(labels)) > 4 and (confidence < 1).any()
    acc = WeightedLabels(grid, n)
    acc.target(target, chains[0], 1, float(target[0].min()))
    for k in range(n):
        acc.add(images[k], maps[k], chains[k], 1, float(images[k][0].min()), 86.0)
    acc.finish()
    for value in want_values:
        p, _, _ = read_volume(one / f"probability_{int(value)}.nii.gz")
        assert same(p, acc.probability(int(value))), value
    assert len(list(one.glob("probability_*.nii.gz"))) == len(want_values)
    with open(one / "segmentation.csv") as fh:
        rows = list(csv.reader(fh))
    found, counts = np.unique(labels, return_counts=True)
    assert rows[0] == ["label", "voxels", "volume_mm3"] and len(rows) == 1 + len(found)
    for row, value, count in zip(rows[1:], found, counts):
        assert int(row[0]) == value and int(row[1]) == count and float(row[2]) == float(count) * (sl[0] * sl[1] * sl[2])

    # -wt 1: VolumeTransform's files
    for source, written, extra in (("target.nii.gz", "transformedTarget.nii.gz", ["-t", "transforms/0.json"]),
                                   (image_names[2], "transformed2.nii.gz", ["-t", "transforms/2.json"]),
                                   (label_names[3], "transformedLabels3.nii.gz", ["-t", "transforms/3.json", "-i", "0", "-b", "86"])):
        r = run([os.path.join(BIN, "VolumeTransform"), source, "dummy.mhd"] + extra + ["-o", "flow.nii.gz"], d)
        assert r.returncode == 0, r.stdout + r.stderr
        a, oa, sa = read_volume(d / "flow.nii.gz")
        b, ob, sb = read_volume(one / written)
        assert same(a, b) and oa == ob and sa == sb, written
    for k in range(n):
        a, o, s = images[k]
        assert same(read_volume(one / f"transformed{k}.nii.gz")[0], chains[k].reslice(a, o, s, *grid, 1, float(a.min()))), k
        a, o, s = maps[k]
        assert same(read_volume(one / f"transformedLabels{k}.nii.gz")[0], chains[k].reslice(a, o, s, *grid, 0, 86.0)), k

    # a float label file: named, exit 1, nothing written; so for a list of the wrong length and an unknown option
    write_volume(d / "float.nii.gz", maps[1][0].astype(np.float32), maps[1][1], maps[1][2])
    (d / "bad.txt").write_text("".join(name + "\n" for name in label_names[:1] + ["float.nii.gz"] + label_names[2:]))
    r = run(tool[:-4] + ["-ll", "bad.txt", "-o", "bad"], d)
    assert r.returncode == 1 and "float.nii.gz" in r.stdout and not (d / "bad").exists(), r.stdout + r.stderr
    (d / "short.txt").write_text("".join(name + "\n" for name in label_names[1:]))
    r = run(tool[:-4] + ["-ll", "short.txt", "-o", "bad"], d)
    assert r.returncode == 1 and "short.txt" in r.stdout and not (d / "bad").exists()
    r = run(tool + ["-o", "bad", "-q", "1"], d)
    assert r.returncode == 1 and "unknown option -q" in r.stdout and not (d / "bad").exists()
    r = run(tool + ["-o", "bad", "-r", "5"], d)
    assert r.returncode == 1 and "-r" in r.stdout and not (d / "bad").exists()
