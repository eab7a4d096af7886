"""Majority-vote label fusion on the device (frog_labels, include/frog_chain.h; bin/FuseLabels; frog_amd.volume.Labels)
against its NumPy restatement (labels_restate.py).  Everything is integer arithmetic or one float32 division: every
comparison is ==."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest

from frog_amd import _abi
from frog_amd.chain import Chain, invert, read_transform
from frog_amd.volume import Labels, bbox_grid, fuse_labels, fused_dtype, group_dice, read_volume, write_volume

import labels_restate

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")
GRID = ((19, 13, 7), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))      # 1729 voxels: seven blocks of 256, the last one partial
TYPES = ("uint8", "int8", "uint16", "int16", "int32", "uint32")
POOL = {"uint8": [0, 58, 86, 170], "int8": [0, 58, 86, -3], "uint16": [0, 58, 86, 170, 1247, 29193, 40358],
        "int16": [0, 58, 86, 170, 1247, 29193], "int32": [0, 58, 86, 170, 1247, 29193, 40358],
        "uint32": [0, 58, 86, 170, 1247, 29193, 40358]}


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def vote_group(kind="radlex"):
    """Six images on GRID, one per integer type, values from the RadLex-like POOL narrowed per type (-3 in the int8 image).
    Slab z = 0 is unanimous, z = 1 has every image different (the winner is the smallest value, -3, with agreement 1/6),
    z = 2 is a 3-3 tie, z = 3 a 2-2-2 tie, the rest is random.
    kind "radlex": as described.  "narrow": 40358 replaced by 1247, so that every value fits int16.
    "wide": 4 000 000 000 in the uint32 image and -2 000 000 000 in the int32 image: no 32-bit type holds both."""
    rng = np.random.default_rng(23)
    shape = GRID[0][::-1]
    vols = []
    for dt in TYPES:
        v = rng.choice(POOL[dt], size=shape)
        v[0] = 58
        vols.append(v)
    for v, value in zip(vols, (170, -3, 40358, 29193, 1247, 86)):
        v[1] = value
    for k, v in enumerate(vols):
        v[2] = 86 if k < 3 else 58
        v[3] = (86, 1247, 0)[k // 2]
    if kind == "narrow":
        for v in vols:
            v[v == 40358] = 1247
    if kind == "wide":
        vols[5][4, :, :9] = 4_000_000_000
        vols[4][5, :, 9:] = -2_000_000_000
    return [v.astype(dt) for v, dt in zip(vols, TYPES)]


def collect(vols, grid=GRID, max_labels=0, dtypes=("int32",)):
    """Every output of an accumulator over `vols` (arrays on the grid): n_labels, the table, fused as each of `dtypes`
    (None where the library refuses the type), the agreement, the probability of every label."""
    acc = Labels(grid, len(vols), max_labels)
    for v in vols:
        acc.add(v)
    out = {"n_labels": acc.finish()}
    out["values"], out["voxels"], out["pairs"] = acc.table()
    for dt in dtypes:
        try:
            out["fused_" + dt], out["agreement"] = acc.fused(dt)
        except _abi.FrogError as e:
            assert e.code == _abi.FROG_E_INVALID
            out["fused_" + dt] = None
    out["agreement_alone"] = agreement_alone(acc)
    out["probability"] = [acc.probability(int(v)) for v in out["values"]]
    out["acc"] = acc
    return out


def agreement_alone(acc):
    a = np.empty(acc.dims[::-1], np.float32)
    _abi.check(acc._lib.frog_labels_fused(acc._h, None, a.ctypes.data_as(_abi.c_float_p)), "frog_labels_fused")
    return a


def assert_matches(out, r, fused=("int32",)):
    assert out["n_labels"] == len(r["values"])
    assert same(out["values"], r["values"]) and same(out["voxels"], r["voxels"]) and same(out["pairs"], r["pairs"])
    for dt in fused:
        assert same(out["fused_" + dt], r["labels"].astype(dt)), dt
    assert same(out["agreement_alone"], r["agreement"])
    if fused:
        assert same(out["agreement"], r["agreement"])
    for l, value in enumerate(r["values"]):
        assert same(out["probability"][l], labels_restate.probability(r, value)), value


def assert_refused_untouched(acc, dtype):
    """frog_labels_fused as `dtype` returns FROG_E_INVALID and writes neither output."""
    import ctypes as C
    labels = np.full(acc.dims[::-1], 77, np.dtype(dtype))
    agreement = np.full(acc.dims[::-1], -5.0, np.float32)
    lv = _abi.volume_view(labels, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    rc = acc._lib.frog_labels_fused(acc._h, C.byref(lv), agreement.ctypes.data_as(_abi.c_float_p))
    assert rc == _abi.FROG_E_INVALID
    assert (labels == 77).all() and (agreement == -5.0).all()


def test_votes_ties_and_types():
    """The issue's first group holds both -3 and 40358, so by the rule it states itself ("a table value that does not fit
    the requested type is refused") only int32 can hold the fused map: int32 is compared with the restatement, int16 and
    uint8 must be refused with the buffers untouched.  The comparison of an int16 fused map is made on the same group with
    40358 replaced by 1247 ("narrow"), where int16 and int32 both hold every value and uint8 still does not."""
    vols = vote_group()
    r = labels_restate.restate(vols)
    assert list(r["values"]) == [-3, 0, 58, 86, 170, 1247, 29193, 40358]
    assert (r["agreement"][0] == 1.0).all() and (r["labels"][0] == 58).all()
    assert (r["labels"][1] == -3).all() and (r["agreement"][1] == np.float32(1) / np.float32(6)).all()
    assert (r["labels"][2] == 58).all() and (r["agreement"][2] == np.float32(0.5)).all()
    assert (r["labels"][3] == 0).all() and (r["agreement"][3] == np.float32(2) / np.float32(6)).all()
    out = collect(vols, dtypes=("int32", "int16", "uint8"))
    assert_matches(out, r)
    assert out["fused_int16"] is None and out["fused_uint8"] is None
    acc = out["acc"]
    assert_refused_untouched(acc, "uint8")
    assert_refused_untouched(acc, "int16")
    with pytest.raises(_abi.FrogError) as e:
        acc.probability(57)
    assert e.value.code == _abi.FROG_E_INVALID
    assert fused_dtype(out["values"]) == np.dtype("int32")

    vols = vote_group("narrow")
    r = labels_restate.restate(vols)
    assert list(r["values"]) == [-3, 0, 58, 86, 170, 1247, 29193]
    out = collect(vols, dtypes=("int32", "int16", "uint8"))
    assert_matches(out, r, fused=("int32", "int16"))
    assert out["fused_uint8"] is None
    assert_refused_untouched(out["acc"], "uint8")
    assert fused_dtype(out["values"]) == np.dtype("int16")
    assert same(out["acc"].fused()[0], r["labels"].astype("int16"))


def test_values_no_32_bit_type_holds():
    vols = vote_group("wide")
    r = labels_restate.restate(vols)
    assert r["values"][0] == -2_000_000_000 and r["values"][-1] == 4_000_000_000
    out = collect(vols, dtypes=TYPES)
    assert all(out["fused_" + dt] is None for dt in TYPES)
    assert_matches(out, r, fused=())
    for dt in TYPES:
        assert_refused_untouched(out["acc"], dt)
    assert fused_dtype(out["values"]) is None
    with pytest.raises(ValueError):
        out["acc"].fused()


def dump(path):
    """The child of test_launch_splitting: the first group's outputs into an .npz."""
    out = collect(vote_group())
    np.savez(path, n_labels=out["n_labels"], values=out["values"], voxels=out["voxels"], pairs=out["pairs"], fused=out["fused_int32"],
             agreement=out["agreement"], probability=np.stack(out["probability"]))


def test_launch_splitting(tmp_path):
    """FROG_CHAIN_LAUNCH_MAX=256: seven launches per kernel over the grid, one block per launch of the table kernel.  The
    hook is read once per process, hence the child."""
    path = str(tmp_path / "split.npz")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_labels as t; t.dump(%r)" % (ROOT, os.path.join(ROOT, "tests"), path)
    env = dict(os.environ, FROG_CHAIN_LAUNCH_MAX="256")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.load(path)
    want = collect(vote_group())
    ref = labels_restate.restate(vote_group())
    assert_matches(want, ref)
    assert int(got["n_labels"]) == want["n_labels"]
    for key in ("values", "voxels", "pairs", "agreement"):
        assert same(got[key], want[key]), key
    assert same(got["fused"], want["fused_int32"])
    assert same(got["probability"], np.stack(want["probability"]))


def test_counter_width():
    """300 images on three voxels, the last 40 different: votes of 300 and 260, which an 8-bit counter cannot hold."""
    grid = ((3, 1, 1), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    first = np.array([[[58, 86, 1247]]], np.uint16)
    last = np.array([[[58, 0, 86]]], np.uint16)
    vols = [first] * 260 + [last] * 40
    r = labels_restate.restate(vols)
    out = collect(vols, grid)
    assert_matches(out, r)
    assert list(out["values"]) == [0, 58, 86, 1247] and list(out["voxels"]) == [40, 300, 300, 260]
    assert list(out["pairs"]) == [40 * 39 // 2, 300 * 299 // 2, 260 * 259 // 2 + 40 * 39 // 2, 260 * 259 // 2]
    assert same(out["agreement"], (np.array([[[300, 260, 260]]], np.float32) / np.float32(300)))


def many_labels():
    """4096 distinct int32 values: runs of k * 8192 and k * 65536 (multiples of plausible table sizes), negative multiples,
    and odd ones out; three permutations of them on a 16^3 grid."""
    rng = np.random.default_rng(31)
    k = np.arange(1500, dtype=np.int64)
    values = np.concatenate([k * 8192, k[200:] * 65536, -k[1:601] * 8192, rng.choice(np.arange(1, 8192), 696, replace=False)])
    assert len(values) == 4096 == len(np.unique(values)) and np.abs(values).max() < 2 ** 31
    return [rng.permutation(values).reshape(16, 16, 16).astype(np.int32) for _ in range(3)]


def test_many_labels_and_colliding_hashes():
    grid = ((16, 16, 16), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    vols = many_labels()
    r = labels_restate.restate(vols)
    out = collect(vols, grid, max_labels=4096)
    assert out["n_labels"] == 4096
    assert_matches(out, r)
    acc = Labels(grid, 3, 4095)
    with pytest.raises(_abi.FrogError) as e:
        acc.add(vols[0])
    assert e.value.code == _abi.FROG_E_INVALID and "4095" in str(e.value)


def test_a_refused_volume_leaves_nothing_behind():
    grid = ((9, 7, 5), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))          # 315 voxels: two blocks
    rng = np.random.default_rng(41)
    shape = grid[0][::-1]
    good = [rng.choice(p, size=shape).astype(dt) for p, dt in (([0, 58], "uint8"), ([0, 58, 86], "int16"), ([0, 58, 86, 1247], "uint16"))]
    bad = [rng.choice([0, 58, 7, 8, 9], size=shape).astype("uint8"), rng.choice([1247, 11, 12], size=shape).astype("int32")]
    for v, n in zip(good + bad, (2, 3, 4, 5, 3)):
        assert len(np.unique(v)) == n
    acc = Labels(grid, 3, max_labels=4)
    acc.add(good[0])
    with pytest.raises(_abi.FrogError) as e:
        acc.add(bad[0])                                             # 0, 58 and three labels of its own: five
    assert e.value.code == _abi.FROG_E_INVALID and "max_labels = 4" in str(e.value)
    acc.add(good[1])
    with pytest.raises(_abi.FrogError) as e:
        acc.add(bad[1])                                             # three known labels and three new ones
    assert e.value.code == _abi.FROG_E_INVALID
    acc.add(good[2])                                                # the third of n_images = 3: the refused calls did not count
    assert acc.finish() == 4
    clean = collect(good, grid, max_labels=4)
    r = labels_restate.restate(good)
    assert_matches(clean, r)
    values, voxels, pairs = acc.table()
    assert list(values) == [0, 58, 86, 1247]
    assert same(values, clean["values"]) and same(voxels, clean["voxels"]) and same(pairs, clean["pairs"])
    labels, agreement = acc.fused("int32")
    assert same(labels, clean["fused_int32"]) and same(agreement, clean["agreement"])
    for l, v in enumerate(values):
        assert same(acc.probability(int(v)), clean["probability"][l])
    for v in (7, 8, 9, 11, 12):
        with pytest.raises(_abi.FrogError):
            acc.probability(v)


def test_protocol():
    grid = ((5, 4, 3), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    rng = np.random.default_rng(43)
    vols = [rng.choice([0, 58, 86], size=(3, 4, 5)).astype(dt) for dt in ("uint8", "int16")]

    def invalid(call, *args, **kw):
        with pytest.raises(_abi.FrogError) as e:
            call(*args, **kw)
        assert e.value.code == _abi.FROG_E_INVALID

    acc = Labels(grid, 2)
    acc._n_labels = 3
    for getter in (acc.table, lambda: acc.fused("int32"), lambda: acc.probability(0)):
        invalid(getter)                                             # before finish
    acc.add(vols[0])
    invalid(acc.finish)                                             # too few adds
    invalid(acc.table)
    invalid(acc.add, vols[1].astype(np.float32))
    invalid(acc.add, vols[1].astype(np.float64))
    invalid(acc.add, vols[1], None, float("nan"))
    invalid(acc.add, vols[1], None, float("inf"))
    invalid(acc.add, np.zeros((3, 4, 6), np.uint8))                 # not on the grid
    acc.add(vols[1])                                                # none of the refused calls counted
    invalid(acc.add, vols[0])                                       # after n_images
    assert acc.finish() == 3
    invalid(acc.add, vols[0])
    r = labels_restate.restate(vols)
    values, voxels, pairs = acc.table()
    labels, agreement = acc.fused()
    assert labels.dtype == np.uint8
    assert same(values, r["values"]) and same(voxels, r["voxels"]) and same(pairs, r["pairs"])
    assert same(labels, r["labels"].astype(np.uint8)) and same(agreement, r["agreement"])
    assert acc.finish() == 3                                        # again: the same answer


# ---- through transforms, and the tool ------------------------------------------------------------------------------------

U8_VALUES = np.array([0, 58, 86, 170, 12, 200, 33, 99, 250])
I16_VALUES = np.array([0, 58, 86, 170, 1247, 29193, -3, 2000, 77])


def _label_volumes(pairs, d):
    """One blocky label volume per image covering its keypoints: uint8 for even images, int16 for odd ones."""
    po, xyz = pairs.point_offset, pairs.xyz
    names = []
    for i in range(pairs.n_images):
        p = xyz[po[i]:po[i + 1]].astype(np.float64)
        lo, hi = p.min(0) - 10.0, p.max(0) + 10.0
        sp = tuple(float(v) for v in np.round((hi - lo) / 36.0, 3))
        dims = tuple(int(np.ceil((h - l) / s)) + 1 for l, h, s in zip(lo, hi, sp))
        z, y, x = np.meshgrid(*[np.arange(n) for n in dims[::-1]], indexing="ij")
        block = ((x // 5) + 3 * (y // 6) + 7 * (z // 4)) % 9
        v = U8_VALUES[block].astype(np.uint8) if i % 2 == 0 else I16_VALUES[block].astype(np.int16)
        name = f"l{i}.nii.gz" if i % 3 else f"l{i}.mhd"
        write_volume(d / name, v, tuple(float(t) for t in lo), sp)
        names.append(name)
    return names


def run(args, cwd, timeout=300):
    return subprocess.run(args, cwd=cwd, capture_output=True, text=True, timeout=timeout)


def test_fuse_labels_matches_the_per_image_flow(tmp_path, small_pairs):
    d = tmp_path
    small_pairs.write(d / "pairs.bin")
    r = run([os.path.join(BIN, "frog"), "pairs.bin", "-li", "12", "-dl", "2", "-di", "8", "-q", "1"], d)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    names = _label_volumes(small_pairs, d)
    n, spacing = small_pairs.n_images, "6.5"
    r = run([os.path.join(BIN, "DummyVolumeGenerator"), "bbox.json", spacing], d)
    assert r.returncode == 0, r.stdout + r.stderr
    flow = d / "flow"
    flow.mkdir()
    for i, v in enumerate(names):
        r = run([os.path.join(BIN, "VolumeTransform"), v, "dummy.mhd", "-t", f"transforms/{i}.json", "-i", "0", "-b", "0",
                 "-o", f"flow/labels_{i}.nii.gz"], d)
        assert r.returncode == 0, r.stdout + r.stderr
    r = run([os.path.join(BIN, "FuseLabels"), "bbox.json", spacing] + names + ["-o", "one", "-wt", "1", "-p", "1"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "read : " in r.stdout and "device : " in r.stdout and "write : " in r.stdout and "total : " in r.stdout
    one = d / "one"
    per_image = []
    for i in range(n):
        a, oa, sa = read_volume(flow / f"labels_{i}.nii.gz")
        b, ob, sb = read_volume(one / f"transformedLabels{i}.nii.gz")
        assert same(a, b) and oa == ob and sa == sb, i
        assert a.dtype == (np.uint8 if i % 2 == 0 else np.int16)
        per_image.append(a)
    want = labels_restate.restate(per_image)
    assert len(want["values"]) > 9 and want["values"][0] == -3 and (want["agreement"] < 1).any()
    labels, ol, sl = read_volume(one / "labels.nii.gz")
    agreement, oa, sa = read_volume(one / "agreement.nii.gz")
    _, og, sg = read_volume(flow / "labels_0.nii.gz")
    assert ol == oa == og and sl == sa == sg
    assert labels.dtype == np.int16 and same(labels, want["labels"].astype(np.int16))
    assert same(agreement, want["agreement"])
    for value in want["values"]:
        p, _, _ = read_volume(one / f"probability_{int(value)}.nii.gz")
        assert same(p, labels_restate.probability(want, value)), value
    assert len(list(one.glob("probability_*.nii.gz"))) == len(want["values"])
    with open(one / "labels.csv") as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == ["label", "voxels", "mean_volume_mm3", "group_dice"] and len(rows) == 1 + len(want["values"])
    dice = labels_restate.dice(want)
    voxel_mm3 = sl[0] * sl[1] * sl[2]
    for l, row in enumerate(rows[1:]):
        assert int(row[0]) == want["values"][l] and int(row[1]) == want["voxels"][l]
        assert float(row[2]) == float(want["voxels"][l]) * voxel_mm3 / float(n)
        assert float(row[3]) == dice[l]
    assert (dice >= 0).all() and (dice <= 1).all()

    # the Python path: the same arrays from Chain objects
    grid = bbox_grid(d / "bbox.json", float(spacing))
    vols = [read_volume(d / name) for name in names]
    chains = [Chain(invert(read_transform(d / "transforms" / f"{i}.json"))) for i in range(n)]
    got_labels, got_agreement, got_values, got_dice = fuse_labels(vols, chains, grid)
    assert same(got_labels, labels) and same(got_agreement, agreement)
    assert same(got_values, want["values"]) and np.array_equal(got_dice, dice)
    assert same(got_dice, group_dice(want["voxels"], want["pairs"], n))

    # a float label file: named, exit 1, nothing written
    f = read_volume(d / names[1])
    write_volume(d / "float.nii.gz", f[0].astype(np.float32), f[1], f[2])
    r = run([os.path.join(BIN, "FuseLabels"), "bbox.json", spacing] + names[:1] + ["float.nii.gz"] + names[2:] + ["-o", "bad"], d)
    assert r.returncode == 1 and "float.nii.gz" in r.stdout, r.stdout + r.stderr
    assert not (d / "bad").exists()
    # an unknown option is an error
    r = run([os.path.join(BIN, "FuseLabels"), "bbox.json", spacing] + names + ["-o", "bad", "-i", "1"], d)
    assert r.returncode == 1 and "unknown option -i" in r.stdout and not (d / "bad").exists()
