"""The coverage-aware Gaussian on the device (frog_smooth_volume, frog_glm_smooth, include/frog_chain.h; bin/GroupStats -s;
frog_amd.volume.smooth_volume, GroupGLM(smooth=...), group_glm(smooth=...)) against its NumPy restatement (smooth_restate.py)
with the taps frog_smooth_taps gives.  Every f64 line is one rounded operation on both sides: every comparison is == on bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

from frog_amd import _abi
from frog_amd.chain import Chain
from frog_amd.volume import GroupGLM, glm_planes, group_glm, read_volume, smooth_taps, smooth_volume

import glm_restate as G
import smooth_restate as S
from test_gpu_clusters import TOOL_CONS, directory, python_result, run, tool_command, tool_dir  # noqa: F401 (tool_dir: a fixture)
from test_gpu_glm import chained_group, design
from test_gpu_cover import GRID
from test_gpu_rank import NONLINEAR_GRID
from test_smooth import DESIGNED_GRID, DESIGNED_PERMS, DESIGNED_SEED, DESIGNED_SHARES, DESIGNED_SIGMA, designed_case, designed_condition, shares

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F4, F8, U4 = np.float32, np.float64, np.uint32


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return np.array_equal(a.view(U4), b.view(U4)) if a.dtype == F4 else np.array_equal(a, b)


def library_taps(sigma, spacing):
    return [smooth_taps(sigma, s)[1] for s in spacing]


# ---- 1. one volume -------------------------------------------------------------------------------------------------------------

# dims (x, y, z), sigma, spacing (x, y, z), take: none, random holes, or holes with whole rows and planes missing
VOLUME_CASES = {
    "odd": ((37, 21, 13), 1.0, (1.0, 1.0, 1.0), "holes"),                   # radius 3; no dim is a multiple of anything
    "tiny": ((5, 3, 2), 2.0, (1.0, 1.0, 1.0), "none"),                      # radius 6: larger than every dim
    "radius1": ((19, 13, 7), 0.3, (1.0, 1.0, 1.0), "rows"),
    "anisotropic": ((23, 17, 11), 1.0, (0.5, 1.0, 2.0), "rows"),            # radii 6, 3, 2
    "wide": ((9, 70, 5), 21.0, (1.0, 1.0, 1.0), "holes"),                   # radius 63: beyond x and z, inside y
    "blocks": ((131, 67, 43), 1.2, (1.0, 1.0, 1.0), "rows"),                # 377 411 voxels: 1475 blocks, rows and planes cross them
    "finite": ((37, 21, 13), 1.0, (1.0, 1.0, 1.0), "none"),                 # the finite rule alone
}


def volume_case(name):
    dims, sigma, spacing, kind = VOLUME_CASES[name]
    shape = dims[::-1]
    rng = np.random.default_rng(sum(dims))
    x = rng.normal(0, 1, shape).astype(F4)
    flat = x.reshape(-1)
    special = np.array([-0.0, 0.0, 3.0e38, -3.0e38, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1.0], F4)
    at = rng.choice(flat.size, min(3 * len(special), flat.size // 2), replace=False)
    flat[at] = np.resize(special, len(at))
    take = None
    if kind != "none":
        take = (rng.random(shape) >= 0.3).astype(np.uint8) * np.uint8(7)      # a flag is any non-zero value
        if kind == "rows":
            take[:, 1, :] = 0
            take[:, :, 2] = 0
            take[shape[0] // 2] = 0
    return x, take, sigma, spacing


def volume_outputs():
    return {name: smooth_volume(c[0], c[2], c[1], c[3]) for name, c in ((n, volume_case(n)) for n in VOLUME_CASES)}


@pytest.fixture(scope="module")
def device_volumes():
    return volume_outputs()


@pytest.mark.parametrize("name", list(VOLUME_CASES))
def test_smooth_volume_equals_the_restatement(device_volumes, name):
    x, take, sigma, spacing = volume_case(name)
    w3 = library_taps(sigma, spacing)
    on = S.taking(x, take)
    assert on.any() and not on.all() and not np.isfinite(x).all()
    want = S.smooth(x, on, w3)
    got = device_volumes[name]
    assert same(got, want), (name, int((got.view(U4) != want.view(U4)).sum()))
    assert (got.view(U4)[~on] == 0x7FC00000).all() and np.isfinite(got[on]).all()
    if name == "anisotropic":
        assert [len(w) - 1 for w in w3] == [6, 3, 2]
    if name == "radius1":
        assert [len(w) - 1 for w in w3] == [1, 1, 1]


def test_sigma_zero_and_a_voxel_alone_keep_their_values():
    x, take, _, spacing = volume_case("odd")
    on = S.taking(x, take)
    got = smooth_volume(x, 0.0, take, spacing)
    # the value, not the sign of a zero: the sum starts from +0.0, so -0.0 comes back as +0.0
    assert np.array_equal(got[on], x[on]) and (got.view(U4)[~on] == 0x7FC00000).all()
    assert same(got[on], np.where(x[on] == 0, F4(0.0), x[on])) and (x[on].view(U4) == 0x80000000).any()
    alone = np.zeros(x.shape, np.uint8)
    alone[6, 10, 20] = alone[0, 0, 0] = alone[12, 20, 36] = 1
    x[6, 10, 20], x[0, 0, 0], x[12, 20, 36] = 0.1, -7.25, 3.0e38
    got = smooth_volume(x, 1.0, alone)
    assert same(got[alone != 0], x[alone != 0]) and np.isnan(got).sum() == x.size - 3


def test_launch_chunks_change_no_bit(tmp_path, device_volumes):
    """FROG_CHAIN_LAUNCH_MAX is read once per process: a child runs every kernel in chunks of 512 work-items."""
    path = str(tmp_path / "chunks.npz")
    code = ("import sys; sys.path[:0] = [%r, %r]; import numpy as np, test_gpu_smooth as t; "
            "np.savez(%r, **t.volume_outputs(), **t.window_outputs((13, 2)))" % (ROOT, HERE, path))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, FROG_CHAIN_LAUNCH_MAX="512"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    chunked = dict(np.load(path))
    plain = dict(device_volumes, **window_outputs((13, 2)))
    assert sorted(chunked) == sorted(plain)
    for k, v in plain.items():
        assert v.dtype == chunked[k].dtype and v.tobytes() == chunked[k].tobytes(), k


# ---- 2. the accumulator ----------------------------------------------------------------------------------------------------------

SIGMA = 1.0                                                 # on GRID (1 mm): radius 3, so windows of 1 and 2 planes are thinner than it
X12, CONS = design(12, 3), np.array([[0.0, 1, 0], [0, 0, 1]])


def stored_planes(smooth, window=None, n=12):
    """The planes the first n adds of the chained group store on GRID."""
    vols, links, mks = chained_group(n)
    acc = GroupGLM(GRID, X12, window, smooth=smooth)
    try:
        for v, l, m in zip(vols, links, mks):
            acc.add(v, Chain(l), m)
        return np.stack([acc.plane(i) for i in range(n)])
    finally:
        acc.close()


@pytest.fixture(scope="module")
def raw_planes():
    return stored_planes(0.0)


def test_add_stores_the_smoothed_map(raw_planes):
    w3 = library_taps(SIGMA, GRID[2])
    assert [len(w) - 1 for w in w3] == [3, 3, 3]
    missing = raw_planes.view(U4) == 0x7FC00000
    assert missing.any() and not missing.all()
    want = S.smooth_planes(raw_planes, w3)
    got = stored_planes(SIGMA)
    assert same(got, want)
    assert ((got.view(U4) == 0x7FC00000) == missing).all()                  # who takes part does not change
    assert same(stored_planes(0.0), raw_planes)
    # smooth = 0 after a smooth of something: off again, the unsmoothed bits
    vols, links, mks = chained_group(4)
    acc = GroupGLM(GRID, X12, smooth=SIGMA)
    acc.smooth(0.0)
    acc.add(vols[0], Chain(links[0]), mks[0])
    assert same(acc.plane(0), raw_planes[0])
    # after an add the choice is made
    for sigma in (SIGMA, 0.0):
        with pytest.raises(_abi.FrogError) as e:
            acc.smooth(sigma)
        assert e.value.code == _abi.FROG_E_STATE
    with pytest.raises(_abi.FrogError) as e:
        acc.smooth(-1.0)
    assert e.value.code == _abi.FROG_E_INVALID
    acc.add(vols[1], Chain(links[1]), mks[1])
    assert same(acc.plane(1), raw_planes[1])
    acc.close()
    with pytest.raises(_abi.FrogError) as e:
        GroupGLM(GRID, X12, smooth=22.0)                            # a radius of 66
    assert e.value.code == _abi.FROG_E_INVALID


@pytest.mark.parametrize("log", [False, True])
def test_add_jacobian_stores_the_smoothed_map(log):
    """sigma = 5 mm on the 4 mm grid: radius 4.  With the logarithm the comparison is against the restatement of the
    unsmoothed DEVICE planes: the 1-ulp log is then on both sides."""
    from test_gpu_chain import random_chain
    rng = np.random.default_rng(83)
    chains = [Chain(random_chain(rng, 2, 1.0)) for _ in range(3)]
    support = ((12, 11, 8), (14.0, 15.0, 10.0), (4.0, 4.0, 4.0))             # a part of the grid: the rest does not take part
    planes = {}
    for sigma in (0.0, 5.0):
        acc = GroupGLM(NONLINEAR_GRID, np.ones((3, 1)), smooth=sigma)
        for k, c in enumerate(chains):
            acc.add_jacobian(c, support if k else None, log=log)
        planes[sigma] = np.stack([acc.plane(i) for i in range(3)])
        acc.close()
    raw = planes[0.0]
    missing = raw.view(U4) == 0x7FC00000
    assert not missing[0].any() and missing[1].any() and not missing[1].all()
    w3 = library_taps(5.0, NONLINEAR_GRID[2])
    assert [len(w) - 1 for w in w3] == [4, 4, 4]
    assert same(planes[5.0], S.smooth_planes(raw, w3))
    assert not same(planes[5.0], raw)
    # windows of their own give the window's part
    for first, n in ((0, 1), (1, 5), (6, 2), (8, 5)):
        acc = GroupGLM(NONLINEAR_GRID, np.ones((3, 1)), window=(first, n), smooth=5.0)
        acc.add_jacobian(chains[1], support, log=log)
        assert same(acc.plane(0), planes[5.0][1][first:first + n]), (first, n)
        acc.close()


# ---- 3. windows ------------------------------------------------------------------------------------------------------------------

def window_outputs(sizes=(13, 1, 2, 5)):
    """The chained group through group_glm with smoothing, whole and in slabs of 1, 2 and 5 planes (13 = 6 x 2 + 1 = 2 x 5 + 3:
    slabs thinner than the radius of 3, and slabs at both ends of the grid), with 6 permutations and sign flips."""
    vols, links, mks = chained_group()
    chains = [Chain(l) for l in links]
    out = {}
    for planes in sizes:
        r = group_glm(X12, CONS, vols, chains, mks, GRID, "images", min_count=5, fill=-3.0, n_perms=6, seed=8, flip=True, two_sided=True,
                      max_planes=planes, smooth=SIGMA)
        for k, v in r.items():
            out[f"{k}_{planes}"] = v
    return out


def test_windows_give_the_whole_grid(raw_planes):
    smoothed = S.smooth_planes(raw_planes, library_taps(SIGMA, GRID[2]))
    want = G.finish(smoothed, X12, CONS, 5, 0.0, None, -3.0)
    perm, sign = G.draw(12, 6, 8, True, True)
    hi, lo = G.permute(smoothed, X12, CONS, perm, sign, 6, 5)
    assert want[4].any() and not want[4].all()
    assert glm_planes(GRID, 12, smooth=SIGMA) == 13
    out = window_outputs()
    for w in (13, 1, 2, 5):
        for name, value in zip(("beta", "sigma", "t", "count", "fit"), want):
            assert same(out[f"{name}_{w}"], value), (name, w)
        assert same(out[f"max_t_{w}"], hi) and same(out[f"min_t_{w}"], lo), w          # the slabs' extrema, combined with max and min
        assert out[f"p_{w}"].tobytes() == out["p_13"].tobytes(), w
    # the planes themselves, in windows of 1, 2 and 5 planes at both ends and in the middle
    whole = stored_planes(SIGMA, n=3)
    assert same(whole, smoothed[:3])
    for first, n in ((0, 1), (0, 2), (0, 5), (5, 1), (6, 2), (4, 5), (12, 1), (11, 2), (8, 5)):
        assert same(stored_planes(SIGMA, (first, n), n=3), whole[:, first:first + n]), (first, n)


def test_a_scratch_that_does_not_fit_is_refused_with_the_bytes(monkeypatch):
    """FROG_CHAIN_FREE_MAX caps what frog_glm_smooth and frog_glm_smooth_planes count as free, so nothing large is allocated:
    the window of 2 planes with its halo of 3 on each side is 8 planes of 19 x 17 voxels at 36 bytes."""
    need = 8 * 19 * 17 * 36
    acc = GroupGLM(GRID, X12, window=(5, 2))
    monkeypatch.setenv("FROG_CHAIN_FREE_MAX", str(need - 1))
    with pytest.raises(_abi.FrogError) as e:
        acc.smooth(SIGMA)
    text = str(e.value)
    assert e.value.code == _abi.FROG_E_NOMEM and f"needs {need} bytes of device memory, {need - 1} are free" in text, text
    # refused: the accumulator stays unsmoothed
    vols, links, mks = chained_group(1)
    acc.add(vols[0], Chain(links[0]), mks[0])
    monkeypatch.delenv("FROG_CHAIN_FREE_MAX")
    assert same(acc.plane(0), stored_planes(0.0, (5, 2), n=1)[0])
    acc.close()
    acc = GroupGLM(GRID, X12, window=(5, 2))
    monkeypatch.setenv("FROG_CHAIN_FREE_MAX", str(need))
    acc.smooth(SIGMA)                                                       # exactly enough
    acc.close()
    # the planes that fit half of the free bytes WITH the scratch of their halo: p planes of 12 images at 4 bytes and
    # min(p + 6, 13) planes at 36 bytes
    plane = 19 * 17
    for p in (1, 2, 6, 7, 12):
        bytes_of = lambda q: plane * (q * 48 + min(q + 6, 13) * 36)                                # noqa: E731
        monkeypatch.setenv("FROG_CHAIN_FREE_MAX", str(2 * bytes_of(p + 1) - 2))
        assert glm_planes(GRID, 12, smooth=SIGMA) == p, p
    monkeypatch.setenv("FROG_CHAIN_FREE_MAX", str(2 * plane * (48 + 7 * 36) - 2))
    with pytest.raises(_abi.FrogError) as e:
        glm_planes(GRID, 12, smooth=SIGMA)
    assert e.value.code == _abi.FROG_E_INVALID
    assert glm_planes(GRID, 12) == 13                                       # frog_glm_planes stays as it is


# ---- 4. the tool -------------------------------------------------------------------------------------------------------------------

def test_group_stats_smoothing(tool_dir):
    d = tool_dir
    r = run(tool_command(d, "s_whole", "-s", "8"), d)
    assert r.returncode == 0 and "stats : 1 slab of 11 planes" in r.stdout, r.stdout + r.stderr
    assert "smoothed: FWHM 8 mm, sigma 3.39729 mm, radii 3 3 3 voxels" in r.stdout, r.stdout
    r = run(tool_command(d, "s_slabs", "-s", "8", "-rp", "2"), d)
    assert r.returncode == 0 and "stats : 6 slabs of 2 planes" in r.stdout, r.stdout + r.stderr
    whole = directory(d / "s_whole")
    assert directory(d / "s_slabs") == whole                # the slab count changes no byte
    for out, extra in (("s_none", ()), ("s_zero", ("-s", "0"))):
        r = run(tool_command(d, out, *extra), d)
        assert r.returncode == 0 and "smoothed" not in r.stdout, r.stdout + r.stderr
    plain = directory(d / "s_none")
    assert directory(d / "s_zero") == plain and sorted(plain) == sorted(whole)
    assert plain["count.nii.gz"] == whole["count.nii.gz"] and plain["t_0.nii.gz"] != whole["t_0.nii.gz"]
    # the Python results, bit for bit
    grid, res = python_result(d, smooth=8 / S.FWHM)
    for name, want in (("t_0.nii.gz", res["t"][0]), ("t_1.nii.gz", res["t"][1]), ("fwe_p_0.nii.gz", res["p"][0]), ("sigma.nii.gz", res["sigma"]),
                       ("beta_1.nii.gz", res["beta"][1]), ("count.nii.gz", res["count"])):
        assert same(read_volume(d / "s_whole" / name)[0], want), name
    # refused before anything is written: negative, not a number, a radius of 3 * 127.4 / 4 = 96 voxels
    for k, value in enumerate(("-1", "abc", "4mm", "nan", "inf", "300", "")):
        r = run(tool_command(d, f"s_bad{k}", "-s", value), d)
        assert r.returncode != 0 and not (d / f"s_bad{k}").exists(), value


# ---- 5. the designed case ----------------------------------------------------------------------------------------------------------

def test_designed_case_on_the_device():
    vols, on, X, con, block = designed_case()
    found = []
    for sigma in (0.0, DESIGNED_SIGMA):
        r = group_glm(X, con, list(vols), None, list(on), DESIGNED_GRID, "images", n_perms=DESIGNED_PERMS, seed=DESIGNED_SEED, smooth=sigma)
        found.append(shares(r["p"][0], block))
    print("designed case on the device: unsmoothed", found[0], "smoothed", found[1])
    designed_condition(*found)
    assert tuple(found) == DESIGNED_SHARES
