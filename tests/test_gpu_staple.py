"""STAPLE label fusion on the device (frog_staple, include/frog_chain.h; bin/FuseLabels -s 1; frog_amd.volume.Staple) against
its NumPy restatement (staple_restate.py).  Every f64 line is one rounded operation on both sides and every sum an exact
u64: every comparison is ==, on every output."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest

from frog_amd import _abi
from frog_amd.chain import Chain, Link, invert, read_transform
from frog_amd.volume import Labels, Staple, bbox_grid, read_volume, robust_z, staple_accuracy, staple_labels

import staple_restate as sr
from test_gpu_labels import GRID, TYPES, _label_volumes, run, vote_group

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")
SHAPE = GRID[0][::-1]
KEYS = ("values", "q", "labels", "confidence", "confidence_alone", "theta", "sums", "totals", "prior", "iterations", "change",
        "active_voxels")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def accumulate(vols, grid=GRID, max_labels=0):
    acc = Staple(grid, len(vols), max_labels)
    for v in vols:
        acc.add(v)
    acc.finish()
    return acc


def outputs(acc, **solve):
    """Every output of one solve on `acc`: q from the probability of every label as (double)q 2^-30 rounded to float32, which
    is exact for q <= 2^30 only in its upper 24 bits -- so the q planes are compared as those float32, and through the sums."""
    out = {}
    out["iterations"], out["change"], out["active_voxels"] = acc.solve(**solve)
    out["values"] = acc.values()
    out["labels"], out["confidence"] = acc.fused("int32")
    alone = np.empty(acc.dims[::-1], np.float32)
    _abi.check(acc._lib.frog_staple_fused(acc._h, None, alone.ctypes.data_as(_abi.c_float_p)), "frog_staple_fused")
    out["confidence_alone"] = alone
    out["q"] = np.stack([acc.probability(int(v)).ravel() for v in out["values"]])
    out["theta"], out["sums"], out["totals"], out["prior"] = acc.performance()
    return out


def expected(vols, **solve):
    r = sr.restate(vols, **solve)
    shape = np.asarray(vols[0]).shape
    return {"values": r["values"], "q": np.stack([sr.probability(r, v) for v in r["values"]]),
            "labels": r["labels"].astype(np.int32).reshape(shape), "confidence": r["confidence"].reshape(shape),
            "confidence_alone": r["confidence"].reshape(shape), "theta": r["theta"], "sums": r["sums"], "totals": r["totals"],
            "prior": r["prior"], "iterations": r["iterations"], "change": r["change"], "active_voxels": r["active_voxels"]}


def assert_same(got, want):
    for key in KEYS:
        if key in ("iterations", "active_voxels"):
            assert got[key] == want[key], key
        elif key == "change":
            assert same(np.float64(got[key]), np.float64(want[key])), (key, got[key], want[key])
        else:
            assert same(got[key], want[key]), key


def check(vols, grid=GRID, **solve):
    acc = accumulate(vols, grid)
    got = outputs(acc, **solve)
    assert_same(got, expected(vols, **solve))
    acc.close()
    return got


@pytest.mark.parametrize("n, error", [(5, 0.3), (6, 0.45)])
@pytest.mark.parametrize("restrict", [False, True])
def test_soft_groups_iteration_by_iteration(n, error, restrict):
    """Every voxel has fractional q; one accumulator, solved with max_iter 0, 1, 2 and 10: equality after every count."""
    truth, vols = sr.noisy_group(n, error)
    vols = [v.astype(np.int16) for v in vols]
    acc = accumulate(vols)
    for max_iter in (0, 1, 2, 10):
        want = expected(vols, max_iter=max_iter, restrict=restrict)
        assert want["iterations"] == max_iter
        assert_same(outputs(acc, max_iter=max_iter, restrict=restrict), want)
    soft = (want["q"] > 0) & (want["q"] < 1)
    assert soft.any(0).mean() > 0.5
    acc.close()


def test_forty_images_to_convergence():
    """n = 40 at 60 %: three renormalisations per product, and the iteration count of the converged run."""
    truth, vols = sr.noisy_group(40, 0.6)
    got = check([v.astype(np.uint8) for v in vols])
    assert 2 < got["iterations"] < 50 and got["change"] < 1e-6


def test_six_hundred_images():
    rates = (0.35 + 0.70 * np.arange(600) / 599.0) * 0.7
    truth, vols = sr.noisy_group(600, rates, cyclic=True)
    got = check([v.astype(np.uint8) for v in vols])
    assert (got["labels"] == truth).all() and (got["theta"] < sr.FLOOR).any()


def spread_values(L):
    """L distinct values spread over int32, negative ones included."""
    return (np.arange(L, dtype=np.int64) - L // 2) * (2 ** 32 // (L + 1) - 7) + 3


@pytest.mark.parametrize("L", [1, 2, 7, 13, 20, 40, 256])
@pytest.mark.parametrize("restrict", [False, True])
def test_label_counts(L, restrict):
    """Every register tile of the E-step alone (L = 1, 2: 4; 7: 8; 13: 16; 20: 32) and tiled (40: a partial second tile; 256:
    eight), and M-step tiles that cut the true labels (256: eleven of 24)."""
    values = spread_values(L)
    assert len(np.unique(values)) == L and values.min() >= -2 ** 31 and values.max() < 2 ** 31
    truth, vols = sr.noisy_group(5, 0.3, L=L, values=values)
    got = check([v.astype(np.int32) for v in vols], max_iter=3, restrict=restrict)
    assert len(got["values"]) == L


def test_unanimous_group_has_nothing_to_solve():
    v = sr.noisy_group(1, 0.0)[1][0].astype(np.int16)
    got = check([v, v.copy(), v.copy()], restrict=True)
    assert got["active_voxels"] == 0 and got["iterations"] == 0 and got["change"] == float("inf")
    assert (got["labels"] == v).all() and (got["confidence"] == 1.0).all()
    got = check([v, v.copy(), v.copy()])
    assert got["active_voxels"] == v.size and (got["labels"] == v).all()


def test_types_and_sparse_values():
    """vote_group: six images, one per integer type, RadLex-like values with -3 and 40358; fused in every type that holds
    them, refused with the buffers untouched in those that do not."""
    import ctypes as C
    vols = vote_group()
    acc = accumulate(vols)
    want = expected(vols)
    assert list(want["values"]) == [-3, 0, 58, 86, 170, 1247, 29193, 40358]
    assert_same(outputs(acc), want)
    for dt in TYPES:
        labels = np.full(acc.dims[::-1], 77, np.dtype(dt))
        confidence = np.full(acc.dims[::-1], -5.0, np.float32)
        lv = _abi.volume_view(labels, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
        rc = acc._lib.frog_staple_fused(acc._h, C.byref(lv), confidence.ctypes.data_as(_abi.c_float_p))
        assert rc == (_abi.FROG_OK if dt == "int32" else _abi.FROG_E_INVALID), dt
        if dt != "int32":
            assert (labels == 77).all() and (confidence == -5.0).all()
    acc.close()
    narrow = vote_group("narrow")
    acc = accumulate(narrow)
    want = sr.restate(narrow)
    acc.solve()
    for dt in ("int16", "int32"):
        assert same(acc.fused(dt)[0], want["labels"].astype(dt).reshape(SHAPE)), dt
    assert acc.fused()[0].dtype == np.int16
    acc.close()


def test_chains_reslice_as_frog_chain_reslice():
    rng = np.random.default_rng(11)
    src_shape, grid = (10, 11, 12), ((19, 17, 13), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    vols, resliced, chains = [], [], []
    acc = Staple(grid, 3)
    for k in range(3):
        M = np.eye(4)
        M[0, 1], M[1, 2] = 0.03125 * k, -0.015625 * k
        M[:3, 3] = [-2.5 - k, -1.25 * k, -0.5]
        chain = Chain([Link.linear(M)])
        v = rng.choice([0, 58, 1247], size=src_shape).astype(np.int16)
        out = acc.add((v, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), chain, 58.0, resliced=True)
        want = chain.reslice(v, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), grid[0], grid[1], grid[2], 0, 58.0)
        assert same(out, want), k
        resliced.append(want)
    acc.finish()
    got = outputs(acc)
    assert_same(got, expected(resliced))
    acc.close()


def test_a_refused_volume_leaves_nothing_behind():
    rng = np.random.default_rng(19)
    vols = [rng.permutation(np.arange(np.prod(SHAPE)) % 256).reshape(SHAPE).astype(np.int16) for _ in range(3)]
    bad = vols[1].copy()
    bad[0, 0, 0] = 1000                                             # the 257th label
    acc = Staple(GRID, 3)
    acc.add(vols[0])
    with pytest.raises(_abi.FrogError) as e:
        acc.add(bad)
    assert e.value.code == _abi.FROG_E_INVALID and "max_labels = 256" in str(e.value)
    acc.add(vols[1])
    acc.add(vols[2])
    assert acc.finish() == 256
    assert_same(outputs(acc, max_iter=2), expected(vols, max_iter=2))
    with pytest.raises(_abi.FrogError):
        acc.probability(1000)
    acc.close()


def test_protocol():
    truth, vols = sr.noisy_group(2, 0.3)
    vols = [v.astype(np.uint8) for v in vols]

    def invalid(call, *args, **kw):
        with pytest.raises(_abi.FrogError) as e:
            call(*args, **kw)
        assert e.value.code == _abi.FROG_E_INVALID

    acc = Staple(GRID, 2)
    acc._n_labels = 4
    invalid(acc.solve)                                              # before finish
    acc.add(vols[0])
    invalid(acc.finish)
    invalid(acc.add, vols[1].astype(np.float32))
    invalid(acc.add, vols[1], None, float("nan"))
    invalid(acc.add, np.zeros((3, 4, 6), np.uint8))
    acc.add(vols[1])
    invalid(acc.add, vols[0])
    assert acc.finish() == 4 and acc.finish() == 4
    for getter in (lambda: acc.fused("int32"), lambda: acc.probability(0), acc.performance):
        invalid(getter)                                             # before solve
    for p0 in (0.0, 1.0, -0.5, 1.5, float("nan")):
        invalid(acc.solve, p0)
    for tol in (-1e-9, float("nan")):
        invalid(acc.solve, 0.99, tol)
    assert_same(outputs(acc, p0=0.9, tol=0.0, max_iter=4), expected(vols, p0=0.9, tol=0.0, max_iter=4))
    acc.close()


def dump(path):
    """The child of test_launch_cutting: a soft group's and a 256-label group's outputs into an .npz."""
    out = {}
    for name, vols, solve in cut_cases():
        got = outputs(accumulate(vols), **solve)
        out.update({f"{name}_{k}": np.asarray(got[k]) for k in KEYS})
    np.savez(path, **out)


def cut_cases():
    a = [v.astype(np.int16) for v in sr.noisy_group(6, 0.45)[1]]
    b = [v.astype(np.int32) for v in sr.noisy_group(5, 0.3, L=256, values=spread_values(256))[1]]
    return [("soft", a, {"restrict": True}), ("wide", b, {"max_iter": 2})]


def test_launch_cutting(tmp_path):
    """FROG_CHAIN_LAUNCH_MAX=512: two blocks per launch of every kernel.  The hook is read once per process, hence the child."""
    path = str(tmp_path / "cut.npz")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_staple as t; t.dump(%r)" % (ROOT, os.path.join(ROOT, "tests"), path)
    env = dict(os.environ, FROG_CHAIN_LAUNCH_MAX="512")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    cut = np.load(path)
    for name, vols, solve in cut_cases():
        want = outputs(accumulate(vols), **solve)
        assert_same({k: cut[f"{name}_{k}"] if cut[f"{name}_{k}"].ndim else cut[f"{name}_{k}"][()] for k in KEYS}, want)


def test_repeatable_and_solvable_again():
    truth, vols = sr.noisy_group(6, 0.45)
    vols = [v.astype(np.int16) for v in vols]
    first, second = outputs(accumulate(vols)), outputs(accumulate(vols))
    assert_same(first, second)
    acc = accumulate(vols)
    outputs(acc)
    again = outputs(acc, p0=0.8, tol=1e-3, max_iter=7, restrict=True)
    assert_same(again, outputs(accumulate(vols), p0=0.8, tol=1e-3, max_iter=7, restrict=True))
    assert_same(again, expected(vols, p0=0.8, tol=1e-3, max_iter=7, restrict=True))


def test_designed_group_on_the_device():
    truth, vols, R = sr.designed_group()
    r = staple_labels(vols)
    assert (r["labels"] == truth).all() and r["labels"].dtype == np.uint8
    acc = Labels(GRID, len(vols))
    for v in vols:
        acc.add(v)
    acc.finish()
    vote = acc.fused()[0]
    assert (vote[R] != truth[R]).all()
    assert np.argmin(r["accuracy"]) >= 2 and r["accuracy"][:2].min() > r["accuracy"][2:].max()
    want = sr.restate(vols)
    assert same(r["accuracy"], staple_accuracy(want["sums"], want["totals"])) and same(r["theta"], want["theta"])


def test_indices_past_2_32():
    """n V = 2049 x 2^21 bytes of D: the plane of the last image lies wholly past 2^32, and it alone disagrees, at 1000
    voxels.  With restrict only those are active, so the restatement is cheap; every inactive voxel has q = ONE."""
    dims = (128, 128, 128)
    grid = (dims, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    rng = np.random.default_rng(13)
    z, y, x = np.meshgrid(*[np.arange(s, dtype=np.uint8) for s in dims[::-1]], indexing="ij")
    base = ((x // 32) + (y // 64) * 2) % 3
    last = base.copy()
    where = rng.choice(base.size, 1000, replace=False)
    last.ravel()[where] = (base.ravel()[where] + 1) % 3
    vols = [base] * 2048 + [last]
    assert len(vols) * base.size > 2 ** 32
    got = check(vols, grid, restrict=True, max_iter=3)
    assert got["active_voxels"] == 1000
    assert (got["labels"] == base).all()


# ---- the tool ----------------------------------------------------------------------------------------------------------------

def test_fuse_labels_tool_with_and_without_staple(tmp_path, small_pairs):
    d = tmp_path
    small_pairs.write(d / "pairs.bin")
    r = run([os.path.join(BIN, "frog"), "pairs.bin", "-li", "12", "-dl", "2", "-di", "8", "-q", "1"], d)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    names = _label_volumes(small_pairs, d)
    n, spacing, bad = small_pairs.n_images, "6.5", 3
    v, o, s = read_volume(d / names[bad])                           # the planted bad image: its label map mirrored along x
    from frog_amd.volume import write_volume
    write_volume(d / names[bad], np.ascontiguousarray(v[:, :, ::-1]), o, s)
    tool = [os.path.join(BIN, "FuseLabels"), "bbox.json", spacing] + names
    r = run(tool + ["-o", "one", "-p", "1"], d)
    assert r.returncode == 0 and "staple" not in r.stdout, r.stdout + r.stderr
    plain = sorted(p.name for p in (d / "one").iterdir())
    assert {"labels.nii.gz", "agreement.nii.gz", "labels.csv"} <= set(plain)
    assert all(p in ("labels.nii.gz", "agreement.nii.gz", "labels.csv") or p.startswith("probability_") for p in plain)
    r = run(tool + ["-o", "two", "-p", "1", "-s", "1", "-sr", "1"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    for p in plain:                                                 # what the tool wrote without -s, byte for byte
        assert (d / "one" / p).read_bytes() == (d / "two" / p).read_bytes(), p
    line = [l for l in r.stdout.splitlines() if l.startswith("staple : ")]
    assert len(line) == 1

    grid = bbox_grid(d / "bbox.json", float(spacing))
    vols = [read_volume(d / name) for name in names]
    chains = [Chain(invert(read_transform(d / "transforms" / f"{i}.json"))) for i in range(n)]
    want = staple_labels(vols, chains, grid, restrict=True)
    assert line[0] == "staple : %d iterations, change %.17g, %d active voxels" % (want["iterations"], want["change"], want["active_voxels"])
    labels, ol, sl = read_volume(d / "two" / "staple.nii.gz")
    vote, ov, sv = read_volume(d / "two" / "labels.nii.gz")
    confidence, _, _ = read_volume(d / "two" / "staple_confidence.nii.gz")
    assert labels.dtype == vote.dtype == np.int16 and ol == ov and sl == sv
    assert same(labels, want["labels"]) and same(confidence, want["confidence"])
    acc = Staple(grid, n)
    for k, vol in enumerate(vols):
        acc.add(vol, chains[k])
    acc.finish()
    acc.solve(restrict=True)
    for value in want["values"]:
        p, _, _ = read_volume(d / "two" / f"staple_probability_{int(value)}.nii.gz")
        assert same(p, acc.probability(int(value))), value
    acc.close()
    with open(d / "two" / "staple.csv") as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == ["label", "prior", "voxels", "volume_mm3"] and len(rows) == 1 + len(want["values"])
    for l, row in enumerate(rows[1:]):
        voxels = int((want["labels"] == want["values"][l]).sum())
        assert int(row[0]) == want["values"][l] and float(row[1]) == want["prior"][l] and int(row[2]) == voxels
        assert float(row[3]) == float(voxels) * (sl[0] * sl[1] * sl[2])
    with open(d / "two" / "performance.csv") as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == ["image", "file", "accuracy", "accuracy_robust_z"] + [f"sensitivity_{int(v)}" for v in want["values"]]
    z = robust_z(want["accuracy"])
    for i, row in enumerate(rows[1:]):
        assert int(row[0]) == i and row[1] == names[i]
        assert float(row[2]) == want["accuracy"][i] and float(row[3]) == z[i]
        assert [float(x) for x in row[4:]] == [want["theta"][i, l, l] for l in range(len(want["values"]))]
    accuracy = [float(row[2]) for row in rows[1:]]
    assert int(np.argmin(accuracy)) == bad and z[bad] == z.min()

    # the options are checked before anything is written
    for extra in (["-s", "1", "-sp", "1"], ["-s", "1", "-st", "-1"], ["-s", "1", "-sr", "2"], ["-sp", "0.9"], ["-s", "1", "-ml", "257"]):
        r = run(tool + ["-o", "bad"] + extra, d)
        assert r.returncode == 1 and not (d / "bad").exists(), extra
