"""Threshold-free cluster enhancement on the device (frog_tfce_volume and frog_tfce, include/frog_chain.h; frog_amd.volume.tfce,
TfceSink, GroupGLM.permute_tfce, tfce_p and group_glm(tfce=...); bin/GroupStats -tf) against the restatements (tfce_restate.py,
clusters_restate.py, glm_restate.py) and the closed forms of test_tfce.py.  Every comparison is == on bytes."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from frog_amd import _abi
from frog_amd.volume import GroupGLM, TfceSink, read_volume, tfce, tfce_p

import clusters_restate as R
import glm_restate as G
import tfce_restate as T
from test_gpu_clusters import (BITS, CONNECTIVITIES, CONS, GRIDS, MIN_COUNT, N, PERMS, SEED, SHAPE, SINK_GRID, TOOL_PERMS, code_of, directory, keys,
                               python_result, run, same, serpentine, sink_model, tool_command, tool_dir)  # noqa: F401 (tool_dir: a fixture)
from test_tfce import closed, edge_values, mid

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BIN = os.path.join(os.path.dirname(HERE), "bin")
F4, F8 = np.float32, np.float64
DHS = (0.1, 0.25)
EH = ((0.5, 2), (0.5, 1), (1, 2), (1, 1))


# ---- 1. one volume -------------------------------------------------------------------------------------------------------------

def noise(dims, df=10):
    """Student-t noise, as the t-map of a null permutation; one NaN, one +0 and one -0 among it."""
    t = np.random.default_rng(dims[0] + 7 * dims[1]).standard_t(df, dims[::-1]).astype(F4)
    t[0, 0, :3] = (np.nan, 0.0, -0.0)
    return t


def designed_maps(dims, dh):
    nx, ny, nz = dims
    shape = (nz, ny, nx)
    out = {}
    box = np.zeros(shape, F4)
    box[0:2, 1:4, 2:6] = mid(7, dh)                         # alone in the grid, at level 7
    out["box"] = box
    peaks = np.zeros(shape, F4)
    peaks[0, 0:3, 2:14] = mid(3, dh)                        # two peaks on a shared plateau of 36 voxels
    peaks[0, 1, 3:5] = mid(6, dh)
    peaks[0, 1, 9:12] = mid(5, dh)
    out["peaks"] = peaks
    v = edge_values(dh)                                     # exact | below | above (258 each) | extra
    pick = [k + part * 258 for k in (0, 1, 2, 3, 7, 100, 254, 255, 256, 257) for part in range(3)] + list(range(3 * 258, len(v)))
    out["edges"] = np.resize(v[pick], shape)                # neighbours at every level up to the saturated one
    for name, first, second, a, b in (("row_end", (0, 0, nx - 1), (0, 1, 0), 2, 5), ("plane_end", (0, ny - 1, nx - 1), (1, 0, 0), 4, 1)):
        ends = np.zeros(shape, F4)                          # neighbours in memory that are none in space, at different levels
        ends[first], ends[second] = mid(a, dh), mid(b, dh)
        out[name] = ends
    out["noise"] = noise(dims)
    return out


@functools.lru_cache(maxsize=None)
def wanted(dims, name, dh, connectivity, side):
    """(the map, its levels, their extents per level): what every e and h share."""
    t = designed_maps(dims, dh)[name]
    level = T.levels(t, dh, side)
    return t, level, T.level_extents(level, connectivity)


def check_volume(dims, name, dh, connectivity, side=0, pairs=EH, twice=False):
    t, level, extents = wanted(dims, name, dh, connectivity, side)
    for e, h in pairs:
        want = T.enhance(level, dh, e, h, connectivity, extents)
        got, top = tfce(t, dh, e, h, connectivity, side)
        print(dims, name, dh, connectivity, side, e, h, "levels", int(level.max()), "max", float(top), "differing voxels", int((got != want).sum()))
        assert same(got, want) and same(top, want.max(initial=F4(0))), (dims, name, dh, connectivity, side, e, h)
        if twice:                                           # a second run: the same bytes
            again, top2 = tfce(t, dh, e, h, connectivity, side)
            assert same(again, got) and same(top2, top)
    return t, level


def test_the_noise_shows_what_the_enhancement_must_get_right():
    """Without this the union-find is never stressed: many levels, and at the lowest one component that holds most voxels."""
    for dims in GRIDS[:3]:
        t = noise(dims)
        level = T.levels(t, 0.1)
        labels, n, largest = R.components(level >= 1, 26)
        assert level.max() >= 20 and 2 * largest > int((level >= 1).sum()), (dims, int(level.max()), n, largest)
        assert np.isnan(t).any() and (T.levels(t, 0.1, 1) >= 20).any()


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("dims", GRIDS[:3])
def test_volume_equals_the_restatement(dims, connectivity):
    test_the_noise_shows_what_the_enhancement_must_get_right()
    for dh in DHS:
        for name in ("box", "peaks", "edges", "row_end", "plane_end"):
            t, level = check_volume(dims, name, dh, connectivity)
            if name == "edges":
                assert level.max() == 255 and (level == 0).any()
                check_volume(dims, name, dh, connectivity, side=1, pairs=EH[:1])
        check_volume(dims, "noise", dh, connectivity, twice=True)
        check_volume(dims, "noise", dh, connectivity, side=1, pairs=EH[::3])
    # the closed forms, which do not go through the restatement
    for dh in DHS:
        for e, h in EH:
            maps = designed_maps(dims, dh)
            got = tfce(maps["box"], dh, e, h, connectivity)[0]
            n = int((maps["box"] != 0).sum())
            assert (got[maps["box"] != 0] == closed({k: n for k in range(1, 8)}, dh, e, h)).all() and (got[maps["box"] == 0] == 0).all()
            for name, tops in (("row_end", (2, 5)), ("plane_end", (4, 1))):     # two voxels, each alone at every level
                got = tfce(maps[name], dh, e, h, connectivity)[0]
                assert [float(v) for v in got[maps[name] != 0]] == [float(closed({k: 1 for k in range(1, c + 1)}, dh, e, h)) for c in tops]
            got = tfce(maps["peaks"], dh, e, h, connectivity)[0]
            plateau = {k: 36 for k in (1, 2, 3)}
            assert (got[0, 1, 3:5] == closed({**plateau, 4: 2, 5: 2, 6: 2}, dh, e, h)).all()
            assert (got[0, 1, 9:12] == closed({**plateau, 4: 3, 5: 3}, dh, e, h)).all()
            assert (got[maps["peaks"] == mid(3, dh)] == closed(plateau, dh, e, h)).all()


BIG = GRIDS[3]


def test_a_grid_of_many_blocks():
    """67 x 45 x 23: 2168 mask words, nine blocks of a word kernel and 271 of a voxel kernel."""
    check_volume(BIG, "noise", 0.25, 26, pairs=EH[:1], twice=True)
    check_volume(BIG, "noise", 0.1, 6, pairs=EH[3:])
    check_volume(BIG, "box", 0.1, 18, pairs=EH[:1])
    check_volume(BIG, "plane_end", 0.25, 26, pairs=EH[1:2])


def path_positions(mask):
    """The position of every voxel along a path one voxel wide that starts at voxel 0: breadth-first over the faces."""
    pos = np.full(mask.shape, -1, np.int64)
    at, k = (0, 0, 0), 0
    while at is not None:
        pos[at] = k
        k += 1
        nxt = None
        for axis in range(3):
            for step in (-1, 1):
                q = list(at)
                q[axis] += step
                if 0 <= q[axis] < mask.shape[axis] and mask[tuple(q)] and pos[tuple(q)] < 0:
                    nxt = tuple(q)
        at = nxt
    assert (pos >= 0).sum() == mask.sum()
    return pos


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_a_path_whose_level_rises_along_it(connectivity):
    """At level k the mask is the path's tail from the first voxel of level k on: one component whose root is the tail's
    smallest index, at every level another, and long parent chains at each.  The extents are counts, so the closed form needs
    no components."""
    mask = serpentine()
    pos = path_positions(mask)
    top = 24
    level = np.where(mask, 1 + pos * top // int(mask.sum()), 0)
    assert level.max() == top and mask.sum() > 1500
    for dh in DHS:
        t = np.where(mask, ((level + 0.5) * dh), 0.0).astype(F4)
        assert same(T.levels(t, dh), level.astype(np.uint8))
        extent = {k: int((level >= k).sum()) for k in range(1, top + 1)}
        for e, h in EH:
            got, best = tfce(t, dh, e, h, connectivity)
            want = np.zeros(mask.shape, F4)
            for own in range(1, top + 1):
                want[level == own] = closed({k: extent[k] for k in range(1, own + 1)}, dh, e, h)
            assert same(got, want) and same(best, want.max()), (dh, e, h, int((got != want).sum()))


# ---- 2. the sink against the restatement of the model --------------------------------------------------------------------------

DH_SINK = 0.25


def the_sink_model():
    vols, on, X, planes, perm, sign, fits = sink_model()
    return dict(grid=SINK_GRID, vols=vols, on=on, X=X, planes=planes, perm=perm, sign=sign, fits=fits)


@functools.lru_cache(maxsize=None)
def tiny_model():
    """12 volumes on a grid of 5 x 4 x 3 voxels under 17 permutations: with two contrasts and two sides 68 slots, two batches."""
    grid = ((5, 4, 3), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    shape, perms = grid[0][::-1], 17
    rng = np.random.default_rng(SEED + 1)
    X = np.stack([np.ones(N), (np.arange(N) % 2).astype(F8), np.arange(N) - (N - 1) / 2.0], axis=1)
    effect = np.zeros(shape)
    effect[1:, 1:3, 1:4] = 3.0
    vols = (rng.normal(0, 1, (N,) + shape) + effect[None] * X[:, 1, None, None, None]).astype(F4)
    on = (rng.random((N,) + shape) >= 0.1).astype(np.uint8)
    planes = np.where(on != 0, vols, G.NAN)
    perm, sign = G.draw(N, perms, SEED, True, True)
    fits = []
    for k in range(perms):
        fit, _, _, t, _ = G.fit(planes.reshape(N, -1), G.design_rows(X, perm[k], sign[k], BITS), CONS, MIN_COUNT)
        fits.append((fit.reshape(shape), t.reshape((len(CONS),) + shape)))
    return dict(grid=grid, vols=vols, on=on, X=X, planes=planes, perm=perm, sign=sign, fits=fits)


@functools.lru_cache(maxsize=None)
def sink_levels(tiny, dh):
    """[k][c][side] -> the levels the sink must hold: those of the voxels that count towards the extrema, 0 elsewhere."""
    m = tiny_model() if tiny else the_sink_model()
    return [[[np.where(fit & ~np.isnan(tc), T.levels(tc, dh, side), 0).astype(np.uint8) for side in (0, 1)] for tc in t] for fit, t in m["fits"]]


@functools.lru_cache(maxsize=None)
def sink_maps(tiny, dh, e, h, connectivity):
    return [[[T.enhance(level, dh, e, h, connectivity) for level in sides] for sides in cons] for cons in sink_levels(tiny, dh)]


def fill(sink, m, window=None, cuts=None):
    """The group into `sink` over one window, the permutations in the calls `cuts`; the (max_t, min_t) the calls returned,
    which are permute's bits."""
    perm, sign = m["perm"], m["sign"]
    cuts = cuts or ((0, len(perm)),)
    acc = GroupGLM(m["grid"], m["X"], window)
    for v, on in zip(m["vols"], m["on"]):
        acc.add(v, None, on)
    parts = [acc.permute_tfce(sink, CONS, perm[a:b], sign[a:b], [1, 2], MIN_COUNT, first_perm=a) for a, b in cuts]
    plain = acc.permute(CONS, perm, sign, [1, 2], MIN_COUNT)
    acc.close()
    got = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    assert same(got[0], plain[0]) and same(got[1], plain[1])
    return got


def check_sink(sink, tiny, dh, e, h, connectivity, sides):
    levels, maps = sink_levels(tiny, dh), sink_maps(tiny, dh, e, h, connectivity)
    best = sink.finish()
    assert best.dtype == F4 and best.shape == (len(levels), len(CONS), sides)
    for k in range(len(levels)):
        for c in range(len(CONS)):
            for side in range(sides):
                assert same(sink.levels(k, c, side), levels[k][c][side]), (k, c, side)
                got = sink.map(k, c, side)
                assert same(got, maps[k][c][side]), (k, c, side, int((got != maps[k][c][side]).sum()))
                assert same(best[k, c, side], maps[k][c][side].max()), (k, c, side)
    assert same(sink.finish(), best)                        # a second finish, after the maps: the same numbers
    return best


def sink_case(tiny, dh, e, h, connectivity, two_sided):
    m = tiny_model() if tiny else the_sink_model()
    sink = TfceSink(m["grid"], len(m["perm"]), len(CONS), dh, e, h, two_sided, connectivity)
    hi, lo = fill(sink, m)
    want = G.permute(m["planes"], m["X"], CONS, m["perm"], m["sign"], BITS, MIN_COUNT)
    assert same(hi, want[0]) and same(lo, want[1])
    best = check_sink(sink, tiny, dh, e, h, connectivity, 2 if two_sided else 1)
    sink.close()
    return best


def test_the_model_shows_what_the_sink_must_get_right():
    levels = sink_levels(False, DH_SINK)
    flat = [levels[k][c][side] for k in range(PERMS) for c in range(len(CONS)) for side in (0, 1)]
    tops = [int(l.max()) for l in flat]
    assert max(tops) >= 20 and 2 * min(tops) <= max(tops) and len(set(tops)) > 4               # slots leave the walk at different levels
    observed = levels[0][0][0]
    assert (observed[2] > 0).any() and (observed[3] > 0).any()                  # a map across the planes 2 | 3
    assert len(tiny_model()["perm"]) * len(CONS) * 2 > 64


@pytest.mark.parametrize("e,h,connectivity,two_sided", [(0.5, 2, 26, True), (1, 1, 6, True), (0.5, 1, 18, False), (1, 2, 26, False)])
def test_sink_equals_the_restatement(e, h, connectivity, two_sided):
    test_the_model_shows_what_the_sink_must_get_right()
    best = sink_case(False, DH_SINK, e, h, connectivity, two_sided)
    assert (best > 0).any()


def test_more_slots_than_one_batch():
    best = sink_case(True, 0.1, 0.5, 2, 26, True)
    assert best.size == 68 and (best[64 // 4:] > 0).any()   # slots of the second batch


CHILD = "import sys; import test_gpu_tfce as M; M.child(sys.argv[1])"


def child(path):
    """Run by test_every_kernel_in_chunks in a process of its own: a sink on SINK_GRID (819 voxels) and one volume on the 67
    x 45 x 23 grid (2168 mask words), their results into `path`."""
    m = the_sink_model()
    sink = TfceSink(SINK_GRID, PERMS, len(CONS), DH_SINK, 0.5, 2, True, 26)
    hi, lo = fill(sink, m)
    best = sink.finish()
    maps = np.stack([sink.map(k, c, side) for k in range(PERMS) for c in range(len(CONS)) for side in (0, 1)])
    levels = np.stack([sink.levels(k, c, side) for k in range(PERMS) for c in range(len(CONS)) for side in (0, 1)])
    sink.close()
    big, top = tfce(noise(BIG), 0.25, 0.5, 2, 26)
    np.savez(path, hi=hi, lo=lo, best=best, maps=maps, levels=levels, big=big, top=top)


def test_every_kernel_in_chunks(tmp_path):
    """FROG_CHAIN_LAUNCH_MAX=512: two launches for the sink's 819 voxels, five for the large grid's 2168 words, 136 for its
    voxels."""
    env = dict(os.environ, FROG_CHAIN_LAUNCH_MAX="512", PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), HERE] + sys.path))
    path = str(tmp_path / "child.npz")
    r = subprocess.run([sys.executable, "-c", CHILD, path], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.load(path)
    m = the_sink_model()
    want = G.permute(m["planes"], m["X"], CONS, m["perm"], m["sign"], BITS, MIN_COUNT)
    assert same(got["hi"], want[0]) and same(got["lo"], want[1])
    levels, maps = sink_levels(False, DH_SINK), sink_maps(False, DH_SINK, 0.5, 2, 26)
    slots = [(k, c, side) for k in range(PERMS) for c in range(len(CONS)) for side in (0, 1)]
    for i, (k, c, side) in enumerate(slots):
        assert same(got["levels"][i], levels[k][c][side]) and same(got["maps"][i], maps[k][c][side]), (k, c, side)
        assert same(got["best"][k, c, side], maps[k][c][side].max())
    t, level, extents = wanted(BIG, "noise", 0.25, 26, 0)
    big = T.enhance(level, 0.25, 0.5, 2, 26, extents)
    assert same(got["big"], big) and same(got["top"][()], big.max())


# ---- 3. slabs ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("planes,sides", [(2, 2), (4, 1), (1, 2)])
def test_windows_fill_one_level_map(planes, sides):
    m = the_sink_model()
    sink = TfceSink(SINK_GRID, PERMS, len(CONS), DH_SINK, 0.5, 2, sides == 2, 26)
    hi, lo = np.full((PERMS, len(CONS)), -np.inf, F4), np.full((PERMS, len(CONS)), np.inf, F4)
    for first in range(0, SHAPE[0], planes):
        h, l = fill(sink, m, (first, min(planes, SHAPE[0] - first)), ((0, 2), (2, PERMS)) if first % 2 == 0 else ((0, 1), (1, 5), (5, PERMS)))
        hi, lo = np.where(keys(h) > keys(hi), h, hi), np.where(keys(l) < keys(lo), l, lo)
    want = G.permute(m["planes"], m["X"], CONS, m["perm"], m["sign"], BITS, MIN_COUNT)
    assert same(hi, want[0]) and same(lo, want[1])
    check_sink(sink, False, DH_SINK, 0.5, 2, 26, sides)     # the whole-grid run's levels, maps and maxima
    sink.close()


# ---- 4. state and refusals -----------------------------------------------------------------------------------------------------

def test_sink_state_and_refusals():
    m = the_sink_model()
    vols, on, X, perm, sign = m["vols"], m["on"], m["X"], m["perm"], m["sign"]
    sink = TfceSink(SINK_GRID, PERMS, len(CONS), DH_SINK, 0.5, 2, True, 26)
    fill(sink, m, (0, 4))
    assert code_of(sink.finish) == _abi.FROG_E_STATE                                        # five planes are missing
    assert code_of(sink.map, 0, 0, 0) == _abi.FROG_E_STATE
    before = sink.levels(0, 0, 0)
    assert before[:4].any() and not before[4:].any()
    acc = GroupGLM(SINK_GRID, X, (3, 2))                                                    # plane 3 again
    for v, o in zip(vols, on):
        acc.add(v, None, o)
    assert code_of(acc.permute_tfce, sink, CONS, perm, sign, [1, 2], MIN_COUNT) == _abi.FROG_E_STATE
    assert same(sink.levels(0, 0, 0), before)                                               # and nothing was written
    acc.close()
    acc = GroupGLM(SINK_GRID, X, (4, 5))
    for v, o in zip(vols, on):
        acc.add(v, None, o)
    for bad in (dict(first_perm=1), dict(first_perm=PERMS), dict(contrasts=CONS[:1]), dict(contrasts=np.concatenate([CONS, CONS[:1]]))):
        args = dict(contrasts=CONS, first_perm=0)
        args.update(bad)
        assert code_of(acc.permute_tfce, sink, args["contrasts"], perm, sign, [1, 2], MIN_COUNT, first_perm=args["first_perm"]) == _abi.FROG_E_INVALID, bad
    other = TfceSink(((13, 7, 8), SINK_GRID[1], SINK_GRID[2]), PERMS, len(CONS), DH_SINK, 0.5, 2, True, 26)
    assert code_of(acc.permute_tfce, other, CONS, perm, sign, [1, 2], MIN_COUNT) == _abi.FROG_E_INVALID         # a sink of another grid
    other.close()
    acc.permute_tfce(sink, CONS, perm[:5], sign[:5], [1, 2], MIN_COUNT)
    assert code_of(sink.finish) == _abi.FROG_E_STATE                                        # the last permutation lacks planes 4 to 8
    assert same(sink.map(0, 0, 0), sink_maps(False, DH_SINK, 0.5, 2, 26)[0][0][0])          # permutation 0 is complete
    acc.permute_tfce(sink, CONS, perm[5:], sign[5:], [1, 2], MIN_COUNT, first_perm=5)
    acc.close()
    check_sink(sink, False, DH_SINK, 0.5, 2, 26, 2)
    for slot in ((PERMS, 0, 0), (0, len(CONS), 0), (0, 0, 2), (0, 0, -1)):
        assert code_of(sink.levels, *slot) == _abi.FROG_E_INVALID and code_of(sink.map, *slot) == _abi.FROG_E_INVALID, slot
    sink.close()
    one = TfceSink(SINK_GRID, PERMS, len(CONS), DH_SINK, 0.5, 2, False, 26)
    assert code_of(one.levels, 0, 0, 1) == _abi.FROG_E_INVALID                              # one side only
    one.close()


def test_bad_parameters_are_refused():
    good = dict(n_perms=PERMS, n_contrasts=2, dh=0.1, e=0.5, h=2, two_sided=False, connectivity=26)
    TfceSink(SINK_GRID, **good).close()
    for bad in (dict(dh=0.0), dict(dh=-0.1), dict(dh=np.nan), dict(dh=np.inf), dict(dh=1e-60), dict(e=0.3), dict(e=2), dict(e=0), dict(h=0), dict(h=1.5),
                dict(h=3), dict(connectivity=8), dict(connectivity=0), dict(n_perms=0), dict(n_contrasts=0), dict(n_contrasts=9)):
        assert code_of(TfceSink, SINK_GRID, **dict(good, **bad)) == _abi.FROG_E_INVALID, bad       # 1e-60 is 0 as an f32
    assert code_of(TfceSink, ((0, 7, 9), SINK_GRID[1], SINK_GRID[2]), **good) == _abi.FROG_E_INVALID
    assert code_of(TfceSink, ((1 << 12, 1 << 12, 129), SINK_GRID[1], SINK_GRID[2]), **good) == _abi.FROG_E_INVALID          # above 2^31 voxels
    t = noise(GRIDS[0])
    for bad in (dict(dh=0.0), dict(dh=np.nan), dict(e=0.25), dict(h=4), dict(connectivity=7), dict(side=2), dict(side=-1)):
        assert code_of(tfce, t, **bad) == _abi.FROG_E_INVALID, bad
    for other in (t.astype(F8), (t > 0).astype(np.uint8), np.ones(t.shape, np.int32)):
        assert code_of(tfce, other) == _abi.FROG_E_INVALID, other.dtype


def test_levels_that_do_not_fit_are_refused_with_the_bytes():
    """2^32 - 1 permutations of 8 contrasts and 2 sides: 5.7e13 bytes of levels on this grid, more than any device has.  The
    request is refused from the sizes alone, before anything is allocated."""
    with pytest.raises(_abi.FrogError) as e:
        TfceSink(SINK_GRID, 2 ** 32 - 1, 8, 0.1, 0.5, 2, True, 26)
    text = str(e.value)
    slots = (2 ** 32 - 1) * 16
    assert e.value.code == _abi.FROG_E_NOMEM and str(slots) in text and "bytes of device memory" in text and "are free" in text, text
    stride, voxels = 26 * 32, 13 * 7 * 9
    assert str(slots * (stride + 8) + voxels * 16 + 26 * 4) in text, text


# ---- 5. group_glm and the tool -------------------------------------------------------------------------------------------------

TFCE_FILES = ["tfce.csv", "maxtfce.csv"] + [f"{stem}_{c}.nii.gz" for stem in ("tfce", "tfce_p") for c in range(2)]


def test_group_stats_tfce_files(tool_dir):
    d = tool_dir
    r = run(tool_command(d, "tf_whole", "-tf", "1"), d)
    assert r.returncode == 0 and "stats : 1 slab of 11 planes" in r.stdout, r.stdout + r.stderr
    r = run(tool_command(d, "tf_slabs", "-tf", "1", "-rp", "2"), d)
    assert r.returncode == 0 and "stats : 6 slabs of 2 planes" in r.stdout, r.stdout + r.stderr
    whole = directory(d / "tf_whole")
    assert set(TFCE_FILES) <= set(whole)
    assert directory(d / "tf_slabs") == whole               # the slab count changes no byte
    # without the option: the files of before, with the bytes the run with the option gives them
    r = run(tool_command(d, "tf_plain"), d)
    assert r.returncode == 0, r.stdout + r.stderr
    plain = directory(d / "tf_plain")
    assert sorted(plain) == sorted(set(whole) - set(TFCE_FILES)) and "glm.csv" in plain and "maxt.csv" in plain
    assert all(whole[name] == data for name, data in plain.items())
    # with -ct as well: each set of files as the run with that option alone gives it
    for out, extra in (("tf_ct", ["-ct", "1.5", "-cc", "18"]), ("tf_both", ["-ct", "1.5", "-tf", "1", "-cc", "18"]), ("tf_18", ["-tf", "1", "-cc", "18"])):
        r = run(tool_command(d, out, *extra), d)
        assert r.returncode == 0, r.stdout + r.stderr
    ct, both, tf = directory(d / "tf_ct"), directory(d / "tf_both"), directory(d / "tf_18")
    assert sorted(both) == sorted(set(ct) | set(tf)) and all(both[name] == data for name, data in list(ct.items()) + list(tf.items()))
    assert any(tf[name] != whole[name] for name in TFCE_FILES)                  # -cc applies to -tf
    # the Python results, byte for byte
    grid, res = python_result(d, tfce=True, max_planes=3)
    assert res["max_tfce"].shape == (TOOL_PERMS, 2) and res["max_tfce"].dtype == F4
    rows = np.loadtxt(d / "tf_whole" / "maxtfce.csv", delimiter=",", skiprows=1).reshape(TOOL_PERMS, 2, 3)
    assert same(rows[:, :, 2].astype(F4), res["max_tfce"]) and (rows[:, :, 0] == np.arange(TOOL_PERMS)[:, None]).all() and (rows[:, :, 1] == [0, 1]).all()
    table = (d / "tf_whole" / "tfce.csv").read_text().splitlines()
    assert table[0] == "contrast,peak_tfce,peak_x,peak_y,peak_z,threshold_p05,voxels_p05" and len(table) == 3
    for c in range(2):
        got, o, s = read_volume(d / "tf_whole" / f"tfce_{c}.nii.gz")
        assert same(got, res["tfce"][c]) and got.dtype == F4 and o == grid[1] and s == grid[2] and (got > 0).any()
        assert same(read_volume(d / "tf_whole" / f"tfce_p_{c}.nii.gz")[0], res["tfce_p"][c])
        assert same(res["tfce_p"][c], T.tfce_p(got, res["max_tfce"][:, c])) and same(res["tfce_p"][c], tfce_p(got, res["max_tfce"][:, c]))
        assert same(res["max_tfce"][0, c], got.max())
        # the observed map is the enhancement of the observed t-map's countable voxels
        t = res["t"][c]
        level = np.where(res["fit"] & ~np.isnan(t), T.levels(t, 0.1), 0).astype(np.uint8)
        assert same(got, T.enhance(level, 0.1))
        f = table[1 + c].split(",")
        peak = int(np.argmax(got.reshape(-1)))                                  # the first of equals: the smallest index
        assert int(f[0]) == c and F4(float(f[1])) == got.reshape(-1)[peak]
        assert [int(v) for v in f[2:5]] == [peak % grid[0][0], peak // grid[0][0] % grid[0][1], peak // (grid[0][0] * grid[0][1])]
        assert f[5] == "inf" and int(f[6]) == 0 == int((res["tfce_p"][c] < 0.05).sum())       # 12 permutations: no p below 1 / 12
    _, res18 = python_result(d, tfce=dict(connectivity=18), cluster_threshold=1.5, connectivity=18)
    for c in range(2):
        assert same(read_volume(d / "tf_both" / f"tfce_{c}.nii.gz")[0], res18["tfce"][c])
        assert same(read_volume(d / "tf_both" / f"clusters_{c}.nii.gz")[0], res18["clusters"][c])


def test_two_sided_is_the_two_sides_combined(tool_dir):
    d = tool_dir
    options = ["-tf", "1", "-tfd", "0.25", "-tfe", "1", "-tfh", "1"]
    r = run(tool_command(d, "tf_two", "-two", "1", *options), d)
    assert r.returncode == 0, r.stdout + r.stderr
    par = dict(dh=0.25, e=1, h=1)
    grid, two = python_result(d, tfce=par, two_sided=True)
    _, pos = python_result(d, tfce=par)
    _, neg = python_result(d, cons=[[0.0, -1.0, 0.0], [0.0, 0.0, -1.0]], tfce=par)         # -t, to the bit
    assert same(two["max_tfce"], np.maximum(pos["max_tfce"], neg["max_tfce"])) and (pos["max_tfce"] != neg["max_tfce"]).any()
    rows = np.loadtxt(d / "tf_two" / "maxtfce.csv", delimiter=",", skiprows=1).reshape(TOOL_PERMS, 2, 3)
    assert same(rows[:, :, 2].astype(F4), two["max_tfce"])
    for c in range(2):
        got = read_volume(d / "tf_two" / f"tfce_{c}.nii.gz")[0]
        assert same(got, two["tfce"][c]) and (got > 0).any() and (got < 0).any()
        assert not ((pos["tfce"][c] > 0) & (neg["tfce"][c] > 0)).any()          # a voxel has at most one side
        assert same(np.where(got > 0, got, F4(0)), pos["tfce"][c]) and same(np.where(got < 0, -got, F4(0)), neg["tfce"][c])
        p = read_volume(d / "tf_two" / f"tfce_p_{c}.nii.gz")[0]
        assert same(p, two["tfce_p"][c]) and same(p, T.tfce_p(got, two["max_tfce"][:, c]))


def test_group_stats_refuses_bad_tfce_options(tool_dir):
    d = tool_dir
    tool = [os.path.join(BIN, "GroupStats"), "bbox.json", "4", "design.csv"]
    for k, extra in enumerate((["-tf", "1"], ["-tfd", "0.2", "-np", "5"], ["-tfe", "1", "-np", "5"], ["-tfh", "1", "-np", "5"], ["-cc", "6", "-np", "5"],
                               ["-cc", "6"], ["-np", "5", "-tf", "2"], ["-np", "5", "-tf", "1", "-tfd", "0"], ["-np", "5", "-tf", "1", "-tfd", "-1"],
                               ["-np", "5", "-tf", "1", "-tfd", "nan"], ["-np", "5", "-tf", "1", "-tfd", "inf"], ["-np", "5", "-tf", "1", "-tfe", "0.3"],
                               ["-np", "5", "-tf", "1", "-tfe", "2"], ["-np", "5", "-tf", "1", "-tfh", "3"], ["-np", "5", "-tf", "1", "-tfh", "0.5"],
                               ["-np", "5", "-tf", "1", "-cc", "8"])):
        r = run(tool + ["-o", f"tfbad{k}"] + extra, d)
        assert r.returncode == 1 and "Error : " in r.stdout and not (d / f"tfbad{k}").exists(), extra
