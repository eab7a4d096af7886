"""Joint label fusion on the device (frog_jlabels, include/frog_chain.h; bin/AtlasSegment -j 1; frog_amd.volume.JointLabels)
against its NumPy restatement (joint_restate.py).  The header states every operation and its order, so every comparison is ==
on dtype, shape and bits.  The solve kernel's tile is a run of 8 voxels along x (one row, one plane): the grid 7 x 6 x 5 lies
inside one tile on x and has a seam at every step on y and z, 19 x 9 x 8 is two tiles and a part on x and has voxels whose
whole radius-3 patch is inside the grid."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from frog_amd import _abi
from frog_amd.chain import Chain, Link, invert, read_transform
from frog_amd.volume import CoverAverage, JointLabels, bbox_grid, joint_atlas_segment, read_volume, write_volume

import joint_restate
from test_gpu_chain import random_chain
from test_gpu_labels import POOL, _label_volumes
from test_gpu_wlabels import UNIT, invalid, mixed_group, run, same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")
GRID_A = ((7, 6, 5),) + UNIT
GRID_B = ((19, 9, 8),) + UNIT


def collect(grid, target, atlases, radius, beta, alpha, fill_label=0, chains=None, target_chain=None, max_labels=0, backgrounds=None):
    """Every output of an accumulator: n_labels, values, the fused map as int32 with its confidence, each alone, the
    probability of every label, every weight plane, and the resliced volumes."""
    acc = JointLabels(grid, len(atlases), max_labels, radius, beta, alpha, True)
    bt, bi, bl = backgrounds or (0.0, 0.0, 0.0)
    out = {"resliced_target": acc.target(target, target_chain, 1, bt, resliced=True), "resliced": []}
    for k, (image, labels) in enumerate(atlases):
        out["resliced"].append(acc.add(image, labels, None if chains is None else chains[k], 1, bi, bl, resliced=True))
    out["n_labels"] = acc.finish()
    out["values"] = acc.values()
    out["labels"], out["confidence"] = acc.fused("int32", fill_label)
    labels = np.empty(acc.dims[::-1], np.int32)
    confidence = np.empty(acc.dims[::-1], np.float32)
    lv = _abi.volume_view(labels, *UNIT)
    _abi.check(acc._lib.frog_jlabels_fused(acc._h, fill_label, C.byref(lv), None), "frog_jlabels_fused")
    _abi.check(acc._lib.frog_jlabels_fused(acc._h, fill_label, None, confidence.ctypes.data_as(_abi.c_float_p)), "frog_jlabels_fused")
    out["labels_alone"], out["confidence_alone"] = labels, confidence
    out["probability"] = [acc.probability(int(v)) for v in out["values"]]
    out["weights"] = [acc.weight(k) for k in range(len(atlases))]
    out["acc"] = acc
    return out


def assert_matches(out, r):
    assert out["n_labels"] == len(r["values"]) and same(out["values"], r["values"])
    for k, w in enumerate(r["weights"]):
        assert same(out["weights"][k], w), k
    assert same(out["labels"], r["labels"].astype(np.int32)) and same(out["labels_alone"], out["labels"])
    assert same(out["confidence"], r["confidence"]) and same(out["confidence_alone"], out["confidence"])
    for l, value in enumerate(r["values"]):
        assert same(out["probability"][l], joint_restate.probability(r, value)), value


def plain_group(grid, n, seed=83):
    """(target, [(image, labels)] x n): float32 images that follow the target more or less closely, uint8 labels."""
    rng = np.random.default_rng(seed)
    shape = grid[0][::-1]
    t = rng.integers(0, 1000, shape).astype(np.float32)
    atlases = []
    for m in np.linspace(0.05, 1.0, n):
        image = ((1 - m) * t + m * rng.integers(0, 1000, shape)).astype(np.float32)
        atlases.append((image, rng.choice([0, 58, 86, 170], size=shape).astype(np.uint8)))
    return t, atlases


# ---- 1. every type, radius, beta and alpha against the restatement ---------------------------------------------------------------

@pytest.mark.parametrize("alpha", [0.1, 2.0 ** -20])
@pytest.mark.parametrize("beta", [1, 2])
@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("grid", [GRID_A, GRID_B], ids=["7x6x5", "19x9x8"])
def test_types_radii_betas_and_alphas(grid, radius, beta, alpha):
    target, atlases = mixed_group(grid)
    r = joint_restate.restate(target, atlases, radius, beta, alpha, fill_label=-9)
    assert list(r["values"]) == [-3, 0, 58, 86, 170, 1247, 29193, 40358]
    assert (r["total"] == 0).any() and (r["total"] != 0).any()             # the target's NaN voxels have no vote at all
    assert len(np.unique(r["weights"][0])) > 100 and min(w.min() for w in r["weights"]) < 0      # they vary, and some are negative
    out = collect(grid, target, atlases, radius, beta, alpha, fill_label=-9)
    assert_matches(out, r)
    assert (out["labels"][r["total"] == 0] == -9).all()
    assert same(out["resliced_target"], target)                            # without a chain: the source
    for (image, labels), (ri, rl) in zip(atlases, out["resliced"]):
        assert same(ri, image) and same(rl, labels)


# ---- 2. the sizes of the system ------------------------------------------------------------------------------------------------------

def test_one_atlas_weighs_exactly_one_where_it_is_active():
    target, atlases = mixed_group(GRID_A)
    atlases = atlases[3:4]                                                  # float32, with NaN and inf
    out = collect(GRID_A, target, atlases, 2, 2, 0.1, fill_label=-1)
    active = np.isfinite(target) & np.isfinite(atlases[0][0])
    assert not active.all() and same(out["weights"][0], active.astype(np.float32))
    assert (out["confidence"] == active).all() and (out["labels"][~active] == -1).all()
    assert_matches(out, joint_restate.restate(target, atlases, 2, 2, 0.1, fill_label=-1))


@pytest.mark.parametrize("n, radius", [(32, 1), (32, 2), (11, 1), (20, 2), (25, 1)])
def test_larger_systems(n, radius):
    """32 atlases: the largest system, nine pairs per lane; at radius 2 its planes are read through the cache instead of LDS.
    11, 20 and 25 atlases: the two, four and six pairs per lane of a whole wavefront per voxel."""
    t, atlases = plain_group(GRID_A, n)
    t[2, 3, 4] = np.nan
    atlases[n // 2][0][1, 2, 3] = np.nan
    out = collect(GRID_A, t, atlases, radius, 2, 0.1)
    assert_matches(out, joint_restate.restate(t, atlases, radius, 2, 0.1))


def test_thirty_three_atlases_are_refused():
    invalid(JointLabels, GRID_A, 33)
    JointLabels(GRID_A, 32).close()


# ---- 3. through chains ---------------------------------------------------------------------------------------------------------------

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
    out = collect(grid, target, atlases, 2, 2, 0.1, chains=chains, target_chain=target_chain, backgrounds=(bt, bi, bl))

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
    r = joint_restate.restate(t, on_grid, 2, 2, 0.1, target_inside=t_inside)
    assert 170 in r["values"]
    assert_matches(out, r)


# ---- 4. launch splitting and repeatability ------------------------------------------------------------------------------------------

def dump(path):
    """The child of test_launch_splitting: the mixed group's outputs on GRID_B into an .npz."""
    target, atlases = mixed_group(GRID_B)
    out = collect(GRID_B, target, atlases, 2, 2, 0.1)
    np.savez(path, values=out["values"], labels=out["labels"], confidence=out["confidence"], probability=np.stack(out["probability"]),
             weights=np.stack(out["weights"]))


def test_launch_splitting_and_repeatability(tmp_path):
    """FROG_CHAIN_LAUNCH_MAX=512: two blocks per launch -- the adds in 512-voxel launches, the solve two tiles at a time (216
    tiles on GRID_B).  The hook is read once per process, hence the child."""
    path = str(tmp_path / "split.npz")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_jlabels as t; t.dump(%r)" % (ROOT, os.path.join(ROOT, "tests"), path)
    env = dict(os.environ, FROG_CHAIN_LAUNCH_MAX="512")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.load(path)
    target, atlases = mixed_group(GRID_B)
    first = collect(GRID_B, target, atlases, 2, 2, 0.1)
    second = collect(GRID_B, target, atlases, 2, 2, 0.1)
    for out in (second, {k: got[k] for k in got.files}):
        assert same(out["values"], first["values"]) and same(out["labels"], first["labels"]) and same(out["confidence"], first["confidence"])
        assert same(np.stack(list(out["probability"])), np.stack(first["probability"]))
        assert same(np.stack(list(out["weights"])), np.stack(first["weights"]))


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------

def test_protocol_and_refusals():
    grid = ((5, 4, 3),) + UNIT
    rng = np.random.default_rng(43)
    t = rng.integers(0, 100, (3, 4, 5)).astype(np.int16)
    images = [rng.integers(0, 100, (3, 4, 5)).astype(dt) for dt in ("uint8", "float32")]
    maps = [rng.choice([0, 58, 86], size=(3, 4, 5)).astype(dt) for dt in ("uint8", "int16")]
    acc = JointLabels(grid, 2, 0, 1, 2, 0.5)
    acc._n_labels = 3
    for getter in (acc.values, lambda: acc.fused("int32"), lambda: acc.probability(0), lambda: acc.weight(0)):
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
    invalid(acc.weight, 0)                                          # created without keep_weights
    r = joint_restate.restate(t, list(zip(images, maps)), 1, 2, 0.5)
    labels, confidence = acc.fused()
    assert labels.dtype == np.uint8 and same(acc.values(), r["values"])
    assert same(labels, r["labels"].astype(np.uint8)) and same(confidence, r["confidence"])
    assert acc.finish() == 3                                        # again: the same answer
    assert same(acc.fused()[1], r["confidence"])
    kept = JointLabels(grid, 2, 0, 1, 2, 0.5, True)
    kept.target(t)
    for image, labels in zip(images, maps):
        kept.add(image, labels)
    kept.finish()
    invalid(kept.weight, 2)
    assert same(kept.weight(1), r["weights"][1])


def test_a_refused_atlas_leaves_nothing_behind():
    grid = ((9, 7, 5),) + UNIT                                     # 315 voxels: two blocks of an add
    rng = np.random.default_rng(41)
    shape = grid[0][::-1]
    t = rng.integers(0, 1000, shape).astype(np.float32)
    image = lambda: (t + rng.integers(0, 500, shape)).astype(np.float32)
    good = [(image(), rng.choice(p, size=shape).astype(dt)) for p, dt in (([0, 58], "uint8"), ([0, 58, 86], "int16"), ([0, 58, 86, 1247], "uint16"))]
    bad = [(image(), rng.choice([0, 58, 7, 8, 9], size=shape).astype("uint8")), (image(), rng.choice([1247, 11, 12], size=shape).astype("int32"))]
    acc = JointLabels(grid, 3, 4, 1, 2, 0.1, True)
    acc.target(t)
    acc.add(*good[0])
    e = invalid(acc.add, *bad[0])                                  # 0, 58 and three labels of its own: five
    assert "max_labels = 4" in str(e)
    acc.add(*good[1])
    invalid(acc.add, *bad[1])                                      # three known labels and three new ones
    acc.add(*good[2])                                              # the third of n_images = 3: the refused calls did not count
    assert acc.finish() == 4
    r = joint_restate.restate(t, good, 1, 2, 0.1)
    assert list(acc.values()) == [0, 58, 86, 1247]
    labels, confidence = acc.fused("int32")
    assert same(labels, r["labels"].astype(np.int32)) and same(confidence, r["confidence"])
    for k in range(3):
        assert same(acc.weight(k), r["weights"][k])
    for v in r["values"]:
        assert same(acc.probability(int(v)), joint_restate.probability(r, v))
    for v in (7, 8, 9, 11, 12):
        invalid(acc.probability, v)


# ---- 6. the tool ---------------------------------------------------------------------------------------------------------------------

def test_atlas_segment_joint_matches_the_python_path_and_leaves_the_vote_alone(tmp_path, small_pairs):
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
    common = ["-p", "1", "-f", "-2", "-bl", "86", "-r", "1"]
    r = run(tool + ["-o", "joint", "-j", "1", "-jw", "1", "-ja", "0.25", "-jb", "1"] + common, d)
    assert r.returncode == 0, r.stdout + r.stderr
    joint = d / "joint"

    grid = bbox_grid(d / "bbox.json", float(spacing))
    images = [read_volume(d / name) for name in image_names]
    maps = [read_volume(d / name) for name in label_names]
    chains = [Chain(invert(read_transform(d / "transforms" / f"{i}.json"))) for i in range(n)]
    target = read_volume(d / "target.nii.gz")
    want_labels, want_confidence, want_values, want_weights = joint_atlas_segment(
        target, images, maps, chains, chains[0], grid, radius=1, beta=1, alpha=0.25, label_background=86.0, fill_label=-2, keep_weights=True)
    labels, ol, sl = read_volume(joint / "segmentation.nii.gz")
    confidence, oc, sc = read_volume(joint / "confidence.nii.gz")
    assert ol == oc == tuple(grid[1]) and sl == sc == tuple(grid[2])
    assert labels.dtype == want_labels.dtype and same(labels, want_labels) and same(confidence, want_confidence)
    assert len(np.unique(labels)) > 4
    for k in range(n):
        assert same(read_volume(joint / f"weight_{k}.nii.gz")[0], want_weights[k]), k
    assert len(list(joint.glob("weight_*.nii.gz"))) == n
    acc = JointLabels(grid, n, 0, 1, 1, 0.25)
    acc.target(target, chains[0], 1, float(target[0].min()))
    for k in range(n):
        acc.add(images[k], maps[k], chains[k], 1, float(images[k][0].min()), 86.0)
    acc.finish()
    for value in want_values:
        p, _, _ = read_volume(joint / f"probability_{int(value)}.nii.gz")
        assert same(p, acc.probability(int(value))), value
    assert len(list(joint.glob("probability_*.nii.gz"))) == len(want_values)

    # without -j: the weighted vote's files, byte for byte those of the Python path of the vote (as test_gpu_wlabels holds it)
    from frog_amd.volume import atlas_segment
    r = run(tool + ["-o", "vote"] + common, d)
    assert r.returncode == 0, r.stdout + r.stderr
    vote_labels, vote_confidence, _ = atlas_segment(target, images, maps, chains, chains[0], grid, radius=1, label_background=86.0, fill_label=-2)
    assert same(read_volume(d / "vote" / "segmentation.nii.gz")[0], vote_labels)
    assert same(read_volume(d / "vote" / "confidence.nii.gz")[0], vote_confidence)
    assert not list((d / "vote").glob("weight_*")) and not same(vote_confidence, want_confidence)

    # options of the other method, before any output
    for extra, word in ((["-j", "1", "-pw", "2"], "-pw"), (["-j", "1", "-fl", "0.5"], "-fl"), (["-j", "1", "-r", "4"], "-r"),
                        (["-j", "1", "-jb", "5"], "-jb"), (["-j", "1", "-ja", "0"], "-ja"), (["-jw", "1"], "-jw")):
        r = run(tool + ["-o", "bad"] + extra, d)
        assert r.returncode == 1 and word in r.stdout and not (d / "bad").exists(), extra
