"""The group's average and stdev images on the device (frog_average, include/frog_chain.h): bin/AverageVolumes,
bin/AverageImage against transform.sh's three-tool flow, the Python API, the CPU reslice and the per-image path."""
import os
import subprocess

import numpy as np
import pytest

from frog_amd import _abi
from frog_amd.chain import Chain, Link, invert
from frog_amd.volume import Average, average, read_volume, write_volume

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")


def restate(volumes):
    """AverageVolumes.cxx:47-59, :68-74 in NumPy: float32 a += x / n, s += (x * x) / n in list order, sqrt(s - a * a)."""
    n = np.float32(len(volumes))
    a = np.zeros(volumes[0].shape, np.float32)
    s = np.zeros_like(a)
    for v in volumes:
        x = v.astype(np.float32)
        a += x / n
        s += (x * x) / n
    with np.errstate(invalid="ignore"):
        return a, np.sqrt(s - a * a)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def run(args, cwd, timeout=300):
    r = subprocess.run(args, cwd=cwd, capture_output=True, text=True, timeout=timeout)
    return r


def mixed_volumes(shape=(9, 10, 11), seed=5):
    """u8, i16, i32, f32, f64 on one grid; a slab where the images hold nearly the same value (the integer images the same
    integer, the float images that integer +- 0.01), where the f32 variance rounds negative about every other voxel
    (NaN in the reference's stdev)."""
    rng = np.random.default_rng(seed)
    common = rng.integers(100, 256, shape[1:]).astype(np.float64)
    out = []
    for dt in ("uint8", "int16", "int32", "float32", "float64"):
        if dt == "uint8":
            v = rng.integers(0, 256, shape)
        elif dt == "int16":
            v = rng.integers(-3000, 3000, shape)
        elif dt == "int32":
            v = rng.integers(-2 ** 30, 2 ** 30, shape)             # beyond f32's 24 bits: the cast rounds
        else:
            v = rng.normal(0, 1e3, shape) + rng.uniform(0, 1, shape)
        v = v.astype(dt)
        v[2] = (common + (rng.uniform(-0.01, 0.01, common.shape) if dt.startswith("float") else 0)).astype(dt)
        out.append(v)
    return out


def test_average_volumes_mixed_types(tmp_path):
    vols = mixed_volumes()
    names = ["v0.nii.gz", "v1.mhd", "v2.nii", "v3.nii.gz", "v4.mhd"]
    for k, (v, name) in enumerate(zip(vols, names)):
        write_volume(tmp_path / name, v, (1.5 * k - 4.0, 2.0, -0.5), (1.0 + 0.25 * k, 2.0, 0.5))
    want_a, want_s = restate(vols)
    assert np.isnan(want_s[2]).any() and not np.isnan(want_s).all()
    r = run([os.path.join(BIN, "AverageVolumes")] + names, tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert [l for l in r.stdout.splitlines() if l.startswith("load : ")] == ["load : " + n for n in names]
    got_a, o, s = read_volume(tmp_path / "average.nii.gz")
    got_s, o2, s2 = read_volume(tmp_path / "stdev.nii.gz")
    assert same(got_a, want_a) and same(got_s, want_s)
    assert o == o2 == (-4.0, 2.0, -0.5) and s == s2 == (1.0, 2.0, 0.5)     # the first file's geometry
    # the Python API on the same arrays
    m, sd = average(vols)
    assert same(m, want_a) and same(sd, want_s)
    # a file whose dimensions differ: exit 1, nothing written
    os.remove(tmp_path / "average.nii.gz"); os.remove(tmp_path / "stdev.nii.gz")
    write_volume(tmp_path / "odd.nii.gz", np.zeros((9, 10, 12), np.int16))
    r = run([os.path.join(BIN, "AverageVolumes"), "v0.nii.gz", "odd.nii.gz", "v1.mhd"], tmp_path)
    assert r.returncode == 1 and "odd.nii.gz" in r.stdout, r.stdout + r.stderr
    assert not (tmp_path / "average.nii.gz").exists() and not (tmp_path / "stdev.nii.gz").exists()


def _group_volumes(pairs, d):
    """One volume per image covering its keypoints (int16 for even images, float32 for odd ones)."""
    po, xyz = pairs.point_offset, pairs.xyz
    names = []
    for i in range(pairs.n_images):
        p = xyz[po[i]:po[i + 1]].astype(np.float64)
        lo, hi = p.min(0) - 10.0, p.max(0) + 10.0
        sp = tuple(float(v) for v in np.round((hi - lo) / 36.0, 3))
        dims = tuple(int(np.ceil((h - l) / s)) + 1 for l, h, s in zip(lo, hi, sp))
        z, y, x = np.meshgrid(*[np.arange(n) for n in dims[::-1]], indexing="ij")
        v = 800 + 500 * np.sin(x / (4.0 + i)) * np.cos(y / 5.0) + 7 * z + 60 * i
        v = v.astype(np.int16) if i % 2 == 0 else (v / 7.0).astype(np.float32)
        name = f"v{i}.nii.gz" if i % 3 else f"v{i}.mhd"
        write_volume(d / name, v, tuple(float(t) for t in lo), sp)
        names.append(name)
    return names


@pytest.mark.parametrize("form", ["sidecar", "json"])
def test_average_image_matches_the_three_tool_flow(tmp_path, small_pairs, form):
    d = tmp_path
    small_pairs.write(d / "pairs.bin")
    r = run([os.path.join(BIN, "frog"), "pairs.bin", "-li", "12", "-dl", "2", "-di", "8", "-q", "1"] + (["-j"] if form == "json" else []), d)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    names = _group_volumes(small_pairs, d)
    n, spacing = small_pairs.n_images, "6.5"
    # transform.sh: DummyVolumeGenerator, one VolumeTransform per image, AverageVolumes
    r = run([os.path.join(BIN, "DummyVolumeGenerator"), "bbox.json", spacing], d)
    assert r.returncode == 0, r.stdout + r.stderr
    flow = d / "flow"
    flow.mkdir()
    for i, v in enumerate(names):
        r = run([os.path.join(BIN, "VolumeTransform"), v, "dummy.mhd", "-t", f"transforms/{i}.json", "-o", f"flow/transformed_{i}.nii.gz"], d)
        assert r.returncode == 0, r.stdout + r.stderr
    r = run([os.path.join(BIN, "AverageVolumes")] + [f"transformed_{i}.nii.gz" for i in range(n)], flow)
    assert r.returncode == 0, r.stdout + r.stderr
    # one process
    r = run([os.path.join(BIN, "AverageImage"), "bbox.json", spacing] + names + ["-o", "one", "-wt", "1"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "read : " in r.stdout and "device : " in r.stdout and "write : " in r.stdout
    for name in ("average.nii.gz", "stdev.nii.gz"):
        a, oa, sa = read_volume(flow / name)
        b, ob, sb = read_volume(d / "one" / name)
        assert same(a, b) and oa == ob and sa == sb, name
    mean, _, _ = read_volume(d / "one" / "average.nii.gz")
    assert mean.dtype == np.float32 and np.isfinite(mean).all() and mean.std() > 1.0
    for i in range(n):
        a, oa, sa = read_volume(flow / f"transformed_{i}.nii.gz")
        b, ob, sb = read_volume(d / "one" / f"transformed{i}.nii.gz")
        assert same(a, b) and oa == ob and sa == sb, i
    # a missing transform: named, exit 1, nothing written
    os.rename(d / "transforms" / f"{n - 1}.json", d / f"{n - 1}.json.away")
    r = run([os.path.join(BIN, "AverageImage"), "bbox.json", spacing] + names + ["-o", "missing", "-wt", "1"], d)
    assert r.returncode == 1 and f"transforms/{n - 1}.json" in r.stdout, r.stdout + r.stderr
    assert not (d / "missing").exists()


def _chains(n, seed):
    from test_chain import smooth_chain
    return [smooth_chain(seed=seed + k, amplitude=1.5) for k in range(n)]


def test_python_api_against_per_image_reslice():
    rng = np.random.default_rng(3)
    grid = ((30, 26, 22), (0.0, 2.0, 4.0), (2.0, 2.5, 3.0))
    vols, chains = [], []
    for k, dt in enumerate(("int16", "float32", "uint8", "int16")):
        o, s = (-5.0 + k, 0.0, 2.0), (1.5, 2.0, 1.25)
        vols.append((rng.uniform(0, 200, (50, 36, 52)).astype(dt), o, s))
    links = _chains(len(vols), 11)
    chains = [Chain(invert(l)) for l in links]
    bgs = [-1.0, 0.5, 3.0, -7.0]
    per_image = [c.reslice(v, o, s, grid[0], grid[1], grid[2], 1, bg) for c, (v, o, s), bg in zip(chains, vols, bgs)]
    want = restate(per_image)
    got = average(vols, chains, grid, 1, bgs)
    assert same(got[0], want[0]) and same(got[1], want[1])
    # nearest neighbour, default backgrounds (each volume's minimum), resliced volumes returned by Average.add
    per_image = [c.reslice(v, o, s, grid[0], grid[1], grid[2], 0, float(v.min())) for c, (v, o, s) in zip(chains, vols)]
    acc = Average(grid, len(vols))
    for c, v, want_r in zip(chains, vols, per_image):
        assert same(acc.add(v, c, 0, float(v[0].min()), resliced=True), want_r)
    m, sd = acc.finish()
    want = restate(per_image)
    assert same(m, want[0]) and same(sd, want[1])
    assert same(average(vols, chains, grid, 0)[0], want[0])
    # call-count errors
    acc = Average(grid, 2)
    acc.add(vols[0], chains[0])
    with pytest.raises(_abi.FrogError) as e:
        acc.finish()
    assert e.value.code == _abi.FROG_E_INVALID
    acc.add(vols[1], chains[1])
    with pytest.raises(_abi.FrogError) as e:
        acc.add(vols[2], chains[2])
    assert e.value.code == _abi.FROG_E_INVALID
    acc.finish()
    with pytest.raises(_abi.FrogError) as e:
        Average(grid, 2).add(np.zeros((22, 26, 31), np.float32))            # not on the grid
    assert e.value.code == _abi.FROG_E_INVALID


def test_against_the_cpu_reslice():
    """One slab against the CPU restatement of vtkImageReslice: per image the device is within 1 LSB on < 2e-3 of the
    voxels (test_gpu_chain.py), so the mean is within 1 / n per differing image, on < n * 2e-3 of the voxels."""
    from oracle.oracle_api import chain_reslice
    rng = np.random.default_rng(9)
    grid = ((40, 36, 6), (0.0, 1.0, 30.0), (1.5, 1.5, 1.5))
    z, y, x = np.meshgrid(np.arange(40), np.arange(48), np.arange(56), indexing="ij")
    vols, links = [], _chains(5, 21)
    for k in range(5):
        v = (1000 + 400 * np.sin(x / (5.0 + k)) * np.cos(y / 7.0) + 10 * z + rng.normal(0, 5, x.shape)).astype(np.int16)
        vols.append((v, (-4.0, -2.0, 0.0), (1.5, 1.5, 2.0)))
    bg = -100.0
    m, sd = average(vols, [Chain(invert(l)) for l in links], grid, 1, bg)
    cpu = [np.clip(np.floor(chain_reslice(invert(l), v, o, s, *grid, 1, bg) + 0.5), -32768, 32767) for l, (v, o, s) in zip(links, vols)]
    wm, ws = restate(cpu)
    n = len(vols)
    diff = np.abs(m.astype(np.float64) - wm)
    assert diff.max() <= 1.0 + 1e-3 and (diff > 1e-3).mean() < n * 2e-3
    ok = np.isfinite(ws) & np.isfinite(sd)
    assert (np.abs(sd[ok] - ws[ok]) > 1e-2).mean() < n * 2e-3
    assert (m != bg).any() and (m != m.flat[0]).any()


def test_average_at_volume_size():
    """192^3 int16 grid, 8 images, each through the inverse of a 1 + 3 link chain (as test_reslice_at_volume_size): the
    fused reslice-and-accumulate equals the per-image frog_chain_reslice volumes accumulated in the restatement."""
    rng = np.random.default_rng(2)
    n = 192
    sp = (300.0 / n,) * 3
    grid = ((n, n, n), (0.0, 0.0, 0.0), sp)
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    base = 1000 + 600 * np.sin(x / 7.0) * np.cos(y / 9.0) + 3 * z
    per_image, acc = [], Average(grid, 8)
    for img in range(8):
        M = np.eye(4); M[:3, 3] = rng.uniform(-3, 3, 3)
        links = [Link.linear(M)]
        for k in (4, 8, 8):
            dims = (k + 3, k + 3, k + 3)
            s = tuple(300.0 / k for _ in range(3))
            links.append(Link.bspline(dims, tuple(-v for v in s), s, (1.5 * rng.normal(size=(dims[0] ** 3, 3))).astype(np.float32)))
        c = Chain(invert(links))
        vol = (base + 40 * img).astype(np.int16)
        per_image.append(c.reslice(vol, (0.0, 0.0, 0.0), sp, *grid, 1, -1.0))
        acc.add((vol, (0.0, 0.0, 0.0), sp), c, 1, -1.0)
        c.close()
    m, sd = acc.finish()
    wm, ws = restate(per_image)
    assert same(m, wm) and same(sd, ws)
    assert (per_image[0] == -1).any() and (per_image[0] != -1).mean() > 0.5
