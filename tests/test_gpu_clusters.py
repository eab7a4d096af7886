"""Connected components and the cluster-extent test on the device (frog_components and frog_clusters, include/frog_chain.h;
frog_amd.volume.components, ClusterSink, GroupGLM.permute_clusters and group_glm(cluster_threshold=...); bin/GroupStats -ct)
against the restatements (clusters_restate.py, glm_restate.py).  Every comparison is == on integers or bits."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from frog_amd import _abi
from frog_amd.chain import Chain, invert, read_transform
from frog_amd.volume import ClusterSink, GroupGLM, bbox_grid, cluster_p, components, group_glm, read_volume

import clusters_restate as R
import glm_restate as G

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BIN = os.path.join(os.path.dirname(HERE), "bin")
F4, F8 = np.float32, np.float64
CONNECTIVITIES = (6, 18, 26)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def keys(x):
    """frog_rank's keys of float32 values: their unsigned order is the order of the floats, -0 < +0."""
    u = np.ascontiguousarray(x, F4).view(np.uint32)
    return np.where(u >> 31 != 0, ~u, u ^ np.uint32(0x80000000)).astype(np.int64)


# ---- 1. components -------------------------------------------------------------------------------------------------------------

GRIDS = ((37, 5, 3), (33, 7, 5), (64, 3, 2), (67, 45, 23))  # x, y, z: no x size is a multiple of 32 but 64, whose planes end mid-word


def serpentine():
    """A path one voxel wide through the 33 x 17 x 9 grid: the even rows of the even planes, joined at alternating ends, and the
    planes joined through one voxel of the odd planes at alternating ends.  Rows and planes two apart do not touch at any
    connectivity, so it is one component whose root, voxel 0, is one end of the path."""
    m = np.zeros((9, 17, 33), bool)
    for z in range(0, 9, 2):
        m[z, ::2] = True
        for k, y in enumerate(range(1, 17, 2)):
            m[z, y, 32 if k % 2 == 0 else 0] = True
    for k, z in enumerate(range(1, 9, 2)):
        m[(z,) + ((16, 32) if k % 2 == 0 else (0, 0))] = True
    return m


def designed_masks(dims):
    nx, ny, nz = dims
    shape = (nz, ny, nx)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")

    def of(*voxels):
        m = np.zeros(shape, bool)
        for v in voxels:
            m[v] = True
        return m

    comb = np.zeros(shape, bool)
    comb[:, ::2, ::2] = True                                # the teeth: columns along z, two apart
    comb[-1] = True                                         # joined in the last plane alone
    out = dict(empty=np.zeros(shape, bool), full=np.ones(shape, bool), one=of((nz // 2, ny // 2, nx - 1)),
               row_end=of((0, 0, nx - 1), (0, 1, 0)), plane_end=of((0, ny - 1, nx - 1), (1, 0, 0)),
               edge=of((0, 1, 1), (0, 2, 2)), corner=of((0, 1, 1), (1, 2, 2)), checkerboard=(x + y + z) % 2 == 0, comb=comb)
    for density in (0.1, 0.3, 0.6):                         # 0.3: near the 6-connected percolation threshold
        out[f"random_{density}"] = np.random.default_rng(nx + int(10 * density)).random(shape) < density
    return out


@functools.lru_cache(maxsize=None)
def wanted(dims, name, connectivity):
    mask = serpentine() if name == "serpentine" else designed_masks(dims)[name]
    return (mask,) + R.components(mask, connectivity)


def check_components(dims, name, connectivity):
    mask, labels, n, largest = wanted(dims, name, connectivity)
    got = components(mask.astype(np.uint8), connectivity, largest=True)
    assert same(got[0], labels) and got[1:] == (n, largest), (dims, name, connectivity, got[1:], (n, largest))
    again = components(mask.astype(np.uint8), connectivity, largest=True)
    assert same(again[0], got[0]) and again[1:] == got[1:], (dims, name, connectivity)      # a second run: the same bytes
    return n, largest


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("dims", GRIDS)
def test_components_equal_the_restatement(dims, connectivity):
    counts = {name: check_components(dims, name, connectivity) for name in designed_masks(dims)}
    voxels = dims[0] * dims[1] * dims[2]
    assert counts["empty"] == (0, 0) and counts["full"] == (1, voxels) and counts["one"] == (1, 1)
    # neighbours in memory that are no neighbours in space
    assert counts["row_end"] == (2, 1) and counts["plane_end"] == (2, 1)
    assert counts["edge"] == ((2, 1) if connectivity == 6 else (1, 2))
    assert counts["corner"] == ((1, 2) if connectivity == 26 else (2, 1))
    set_voxels = (voxels + 1) // 2
    if connectivity == 6:
        assert counts["checkerboard"] == (set_voxels, 1)   # every voxel alone
    else:
        assert counts["checkerboard"] == (1, set_voxels)   # the restatement's count: joined through the edges
    teeth = ((dims[0] + 1) // 2) * ((dims[1] + 1) // 2)
    assert counts["comb"] == (1, dims[0] * dims[1] + teeth * (dims[2] - 1))


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_a_long_path_is_one_component(connectivity):
    mask = serpentine()
    n, largest = check_components((33, 17, 9), "serpentine", connectivity)
    assert (n, largest) == (1, int(mask.sum())) and largest > 1500 and mask[0, 0, 0]
    labels = components(mask.astype(np.uint8), connectivity)[0]
    assert same(labels, mask.astype(np.uint32))


def test_every_integer_type_is_a_mask():
    mask = designed_masks(GRIDS[1])["random_0.3"]
    _, labels, n, largest = wanted(GRIDS[1], "random_0.3", 18)
    for dtype, value in (("uint8", 255), ("int8", -128), ("uint16", 256), ("int16", -256), ("uint32", 1 << 16), ("int32", -(1 << 24))):
        got = components(np.where(mask, value, 0).astype(dtype), 18, largest=True)       # values whose low byte is zero count too
        assert same(got[0], labels) and got[1:] == (n, largest), dtype
    assert same(components(mask, 18)[0], labels)            # bool
    for dtype in ("float32", "float64"):
        with pytest.raises(_abi.FrogError) as e:
            components(mask.astype(dtype), 18)
        assert e.value.code == _abi.FROG_E_INVALID


# ---- 2. the sink against the restatement of the model --------------------------------------------------------------------------

SINK_GRID = ((13, 7, 9), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))  # a plane of 91 voxels: no window starts on a word but the first
SHAPE = SINK_GRID[0][::-1]
N, PERMS, SEED, MIN_COUNT, BITS = 12, 6, 23, 5, 0b110
CONS = np.array([[0.0, 1, 0], [0, 0, 1]])
T0 = 4.0                                                    # chosen on the restatement alone: see sink_reference()


def sink_group():
    """12 float volumes on SINK_GRID with on-grid masks, as test_gpu_glm.py builds its groups: noise, a tenth of the entries
    dropped, and a smooth effect of the group column planted in four blobs, two of which span the planes 2 | 3."""
    rng = np.random.default_rng(SEED)
    X = np.stack([np.ones(N), (np.arange(N) % 2).astype(F8), np.arange(N) - (N - 1) / 2.0], axis=1)
    z, y, x = np.meshgrid(np.arange(SHAPE[0]), np.arange(SHAPE[1]), np.arange(SHAPE[2]), indexing="ij")

    def blob(cz, cy, cx, s):
        return np.exp(-((z - cz) ** 2 + (y - cy) ** 2 + (x - cx) ** 2) / (2.0 * s * s))

    effect = 5.0 * (blob(2.5, 3, 3, 1.6) + blob(6, 1, 10, 1.2) - blob(6.5, 5, 5, 1.4) + 0.8 * blob(1, 5, 10, 1.0))
    vols = (rng.normal(0, 1, (N,) + SHAPE) + effect[None] * X[:, 1, None, None, None]).astype(F4)
    on = (rng.random((N,) + SHAPE) >= 0.1).astype(np.uint8)
    return vols, on, X


@functools.lru_cache(maxsize=None)
def sink_model():
    """The group, its permutations, and per permutation the restatement's (fit, t)."""
    vols, on, X = sink_group()
    planes = np.where(on != 0, vols, G.NAN)
    perm, sign = G.draw(N, PERMS, SEED, True, True)
    fits = []
    for k in range(PERMS):
        fit, _, _, t, _ = G.fit(planes.reshape(N, -1), G.design_rows(X, perm[k], sign[k], BITS), CONS, MIN_COUNT)
        fits.append((fit.reshape(SHAPE), t.reshape((len(CONS),) + SHAPE)))
    return vols, on, X, planes, perm, sign, fits


@functools.lru_cache(maxsize=None)
def sink_reference(connectivity=26):
    """[k][c][side] -> (mask, labels, n, largest) from the restatements."""
    fits = sink_model()[6]
    out = []
    for fit, t in fits:
        out.append([[(m,) + R.components(m, connectivity) for m in (fit & ~np.isnan(tc) & (tc > F4(T0)), fit & ~np.isnan(tc) & (tc < -F4(T0)))]
                    for tc in t])
    return out


def fill(sink, window=None, cuts=((0, PERMS),)):
    """The group into `sink` over one window, the permutations in the calls `cuts`; the (max_t, min_t) the calls returned."""
    vols, on, X, _, perm, sign, _ = sink_model()
    acc = GroupGLM(SINK_GRID, X, window)
    for v, m in zip(vols, on):
        acc.add(v, None, m)
    parts = [acc.permute_clusters(sink, CONS, perm[a:b], sign[a:b], [1, 2], MIN_COUNT, first_perm=a) for a, b in cuts]
    plain = acc.permute(CONS, perm, sign, [1, 2], MIN_COUNT)
    acc.close()
    got = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    assert same(got[0], plain[0]) and same(got[1], plain[1])                                # permute's bits
    return got


def check_sink(sink, connectivity=26, sides=2):
    ref = sink_reference(connectivity)
    extents = sink.finish()
    assert extents.dtype == np.uint32 and extents.shape == (PERMS, len(CONS), sides)
    for k in range(PERMS):
        for c in range(len(CONS)):
            for side in range(sides):
                mask, labels, n, largest = ref[k][c][side]
                assert same(sink.mask(k, c, side), mask), (k, c, side)
                assert extents[k, c, side] == largest, (k, c, side)
                got, count = sink.labels(k, c, side)
                assert count == n and same(got, labels), (k, c, side)


def test_the_threshold_shows_what_the_sink_must_get_right():
    ref = sink_reference()
    multi, crossing = 0, 0
    for c in range(len(CONS)):
        for side in range(2):
            _, labels, n, _ = ref[0][c][side]
            for l in range(1, n + 1):
                planes = np.unique(np.nonzero(labels == l)[0])
                multi += int((labels == l).sum() > 1)
                crossing += int(2 in planes and 3 in planes)
    assert multi >= 3 and crossing >= 1                     # under the identity: clusters, one of them across z = 2 | 3
    assert any(not ref[k][c][side][0].any() for k in range(PERMS) for c in range(len(CONS)) for side in range(2))   # an empty side
    assert all(ref[k][c][0][0].any() or ref[k][c][1][0].any() for k in range(1, PERMS) for c in range(len(CONS)))  # no empty permutation


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_sink_equals_the_restatement(connectivity):
    test_the_threshold_shows_what_the_sink_must_get_right()
    sink = ClusterSink(SINK_GRID, PERMS, len(CONS), T0, True, connectivity)
    hi, lo = fill(sink)
    planes, X, perm, sign = sink_model()[3], sink_model()[2], sink_model()[4], sink_model()[5]
    want = G.permute(planes, X, CONS, perm, sign, BITS, MIN_COUNT)
    assert same(hi, want[0]) and same(lo, want[1])
    check_sink(sink, connectivity)
    check_sink(sink, connectivity)                          # a second finish: the same numbers
    sink.close()


# ---- 3. slabs ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("planes,sides", [(2, 2), (4, 1), (1, 2)])
def test_windows_fill_one_mask(planes, sides):
    sink = ClusterSink(SINK_GRID, PERMS, len(CONS), T0, sides == 2, 26)
    hi, lo = np.full((PERMS, len(CONS)), -np.inf, F4), np.full((PERMS, len(CONS)), np.inf, F4)
    for first in range(0, SHAPE[0], planes):
        h, l = fill(sink, (first, min(planes, SHAPE[0] - first)), ((0, 2), (2, PERMS)) if first % 2 == 0 else ((0, PERMS),))
        hi, lo = np.where(keys(h) > keys(hi), h, hi), np.where(keys(l) < keys(lo), l, lo)
    planes_, X, perm, sign = sink_model()[3], sink_model()[2], sink_model()[4], sink_model()[5]
    want = G.permute(planes_, X, CONS, perm, sign, BITS, MIN_COUNT)
    assert same(hi, want[0]) and same(lo, want[1])
    check_sink(sink, 26, sides)
    sink.close()


# ---- 4. state ------------------------------------------------------------------------------------------------------------------

def code_of(call, *args, **kw):
    with pytest.raises(_abi.FrogError) as e:
        call(*args, **kw)
    return e.value.code


def test_sink_state_and_refusals():
    vols, on, X, _, perm, sign, _ = sink_model()
    sink = ClusterSink(SINK_GRID, PERMS, len(CONS), T0, True, 26)
    fill(sink, (0, 4))
    assert code_of(sink.finish) == _abi.FROG_E_STATE                                        # five planes are missing
    assert code_of(sink.labels, 0, 0, 0) == _abi.FROG_E_STATE
    before = sink.mask(0, 0, 0)
    assert before[:4].any() and not before[4:].any()
    acc = GroupGLM(SINK_GRID, X, (3, 2))                                                    # plane 3 again
    for v, m in zip(vols, on):
        acc.add(v, None, m)
    assert code_of(acc.permute_clusters, sink, CONS, perm, sign, [1, 2], MIN_COUNT) == _abi.FROG_E_STATE
    assert same(sink.mask(0, 0, 0), before)                                                 # and nothing was written
    acc.close()
    acc = GroupGLM(SINK_GRID, X, (4, 5))
    for v, m in zip(vols, on):
        acc.add(v, None, m)
    for bad in (dict(first_perm=1), dict(first_perm=PERMS), dict(contrasts=CONS[:1]), dict(contrasts=np.concatenate([CONS, CONS[:1]]))):
        args = dict(contrasts=CONS, first_perm=0)
        args.update(bad)
        assert code_of(acc.permute_clusters, sink, args["contrasts"], perm, sign, [1, 2], MIN_COUNT, first_perm=args["first_perm"]) == _abi.FROG_E_INVALID, bad
    other = ClusterSink(((13, 7, 8), SINK_GRID[1], SINK_GRID[2]), PERMS, len(CONS), T0, True, 26)
    assert code_of(acc.permute_clusters, other, CONS, perm, sign, [1, 2], MIN_COUNT) == _abi.FROG_E_INVALID     # a sink of another grid
    other.close()
    acc.permute_clusters(sink, CONS, perm[:5], sign[:5], [1, 2], MIN_COUNT)
    assert code_of(sink.finish) == _abi.FROG_E_STATE                                        # the last permutation lacks planes 4 to 8
    sink.labels(0, 0, 0)                                                                    # permutation 0 is complete
    acc.permute_clusters(sink, CONS, perm[5:], sign[5:], [1, 2], MIN_COUNT, first_perm=5)
    acc.close()
    check_sink(sink)
    for slot in ((PERMS, 0, 0), (0, len(CONS), 0), (0, 0, 2), (0, 0, -1)):
        assert code_of(sink.mask, *slot) == _abi.FROG_E_INVALID and code_of(sink.labels, *slot) == _abi.FROG_E_INVALID, slot
    sink.close()
    one = ClusterSink(SINK_GRID, PERMS, len(CONS), T0, False, 26)
    assert code_of(one.mask, 0, 0, 1) == _abi.FROG_E_INVALID                                # one side only
    one.close()


def test_masks_whose_bytes_cannot_be_counted_are_refused():
    """2^32 - 1 permutations of 8 contrasts and 2 sides on the largest grid a create accepts, 2^31 voxels: the masks' bytes do
    not fit 64 bits, and a product that wrapped would ask for a few GB.  The request is refused from the sizes alone, before
    anything is allocated."""
    dims = (1 << 11, 1 << 10, 1 << 10)
    voxels = dims[0] * dims[1] * dims[2]
    slots, words = (2 ** 32 - 1) * 16, voxels // 32
    assert voxels == 1 << 31 and slots * (words * 4 + 8) + voxels * 8 >= 2 ** 64 > slots * (words // 2 * 4 + 8) + voxels * 4
    with pytest.raises(_abi.FrogError) as e:
        ClusterSink((dims, SINK_GRID[1], SINK_GRID[2]), 2 ** 32 - 1, 8, T0, True, 26)
    text = str(e.value)
    assert e.value.code == _abi.FROG_E_NOMEM and str(slots) in text and "masks" in text and "more than 2^64" in text and "are free" in text, text
    assert code_of(ClusterSink, ((dims[0] + 1,) + dims[1:], SINK_GRID[1], SINK_GRID[2]), 2 ** 32 - 1, 8, T0, True, 26) == _abi.FROG_E_INVALID


# ---- 5. group_glm and the tool -------------------------------------------------------------------------------------------------

def run(args, cwd, timeout=300):
    return subprocess.run(args, cwd=cwd, capture_output=True, text=True, timeout=timeout)


N_TOOL, TOOL_PERMS, TOOL_SEED, TOOL_T0, SPACING = 8, 12, 9, 1.5, "4"
TOOL_X = np.stack([np.ones(N_TOOL), np.arange(N_TOOL) % 2, np.array([31, 45, 52, 38, 60, 27, 49, 55.0])], axis=1)
TOOL_CONS = [[0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]              # the tool's default contrasts: one per column that is not constant


@pytest.fixture(scope="module")
def tool_dir(tmp_path_factory):
    from test_chain import smooth_chain
    from test_gpu_chain import _write_chain
    d = tmp_path_factory.mktemp("clusters")
    (d / "bbox.json").write_text(json.dumps({"bbox": [[0.0, 0.0, 0.0], [60.0, 52.0, 44.0]]}))
    (d / "transforms").mkdir()
    for i in range(N_TOOL):
        _write_chain(d / "transforms" / f"{i}.json", smooth_chain(seed=70 + i, amplitude=1.5))
    (d / "design.csv").write_text("intercept,group,age\n" + "\n".join(",".join(repr(float(v)) for v in row) for row in TOOL_X) + "\n")
    return d


def tool_command(d, out, *extra):
    return [os.path.join(BIN, "GroupStats"), "bbox.json", SPACING, "design.csv", "-o", out, "-np", str(TOOL_PERMS), "-ps", str(TOOL_SEED)] + list(extra)


def python_result(d, cons=TOOL_CONS, **kw):
    grid = bbox_grid(d / "bbox.json", float(SPACING))
    chains = [Chain(invert(read_transform(d / "transforms" / f"{i}.json"))) for i in range(N_TOOL)]
    return grid, group_glm(TOOL_X, cons, None, chains, None, grid, "logjacobian", n_perms=TOOL_PERMS, seed=TOOL_SEED, **kw)


def directory(path):
    return {name: (path / name).read_bytes() for name in sorted(os.listdir(path))}


def test_group_stats_cluster_files(tool_dir):
    d = tool_dir
    r = run(tool_command(d, "whole", "-ct", str(TOOL_T0)), d)
    assert r.returncode == 0 and "stats : 1 slab of 11 planes" in r.stdout, r.stdout + r.stderr
    r = run(tool_command(d, "slabs", "-ct", str(TOOL_T0), "-rp", "2"), d)
    assert r.returncode == 0 and "stats : 6 slabs of 2 planes" in r.stdout, r.stdout + r.stderr
    whole = directory(d / "whole")
    new = ["clusters.csv", "maxextent.csv"] + [f"{stem}_{c}.nii.gz" for stem in ("clusters", "cluster_p") for c in range(2)]
    assert set(new) <= set(whole)
    assert directory(d / "slabs") == whole                  # the slab count changes no byte
    # without the option: the files of before, with the bytes the run with the option gives them
    for out in ("plain", "again"):
        r = run(tool_command(d, out), d)
        assert r.returncode == 0, r.stdout + r.stderr
    plain = directory(d / "plain")
    assert plain == directory(d / "again") and sorted(plain) == sorted(set(whole) - set(new)) and "glm.csv" in plain and "maxt.csv" in plain
    assert all(whole[name] == data for name, data in plain.items())
    # the Python results, byte for byte
    grid, res = python_result(d, cluster_threshold=TOOL_T0, max_planes=3)
    assert res["max_extent"].shape == (TOOL_PERMS, 2) and res["max_extent"].dtype == np.uint32
    for c in range(2):
        labels, o, s = read_volume(d / "whole" / f"clusters_{c}.nii.gz")
        assert same(labels, res["clusters"][c]) and labels.dtype == np.int32 and o == grid[1] and s == grid[2]
        assert same(read_volume(d / "whole" / f"cluster_p_{c}.nii.gz")[0], res["cluster_p"][c])
        assert same(read_volume(d / "whole" / f"t_{c}.nii.gz")[0], res["t"][c])
    rows = np.loadtxt(d / "whole" / "maxextent.csv", delimiter=",", skiprows=1).reshape(TOOL_PERMS, 2, 3)
    assert (rows[:, :, 2] == res["max_extent"]).all() and (rows[:, :, 0] == np.arange(TOOL_PERMS)[:, None]).all() and (rows[:, :, 1] == [0, 1]).all()
    # clusters.csv follows from clusters_<c>, t_<c> and maxextent.csv
    table = (d / "whole" / "clusters.csv").read_text().splitlines()
    assert table[0] == "contrast,cluster,sign,voxels,peak_t,peak_x,peak_y,peak_z,p_fwe"
    listed = [line.split(",") for line in table[1:]]
    assert len(listed) == sum(int(res["clusters"][c].max()) for c in range(2)) and len(listed) >= 2
    at = 0
    for c in range(2):
        labels, t = res["clusters"][c], res["t"][c]
        assert ((labels > 0) == (res["fit"] & ~np.isnan(t) & (t > F4(TOOL_T0)))).all()
        assert same(np.asarray(res["cluster_extent"][c]), np.bincount(labels.reshape(-1))[1:].astype(np.uint32))
        assert same(labels.astype(np.uint32), R.components(labels > 0, 26)[0])
        for l in range(1, int(labels.max()) + 1):
            f = listed[at]
            at += 1
            member = np.flatnonzero(labels.reshape(-1) == l)
            peak = member[np.argmax(np.abs(t.reshape(-1)[member]))]             # the first of equals: the smallest index
            p = F4((1 + int((rows[1:, c, 2] >= len(member)).sum())) / F8(TOOL_PERMS))
            assert [int(v) for v in f[:4]] == [c, l, 1, len(member)]
            assert F4(float(f[4])) == t.reshape(-1)[peak] and [int(v) for v in f[5:8]] == [peak % grid[0][0], peak // grid[0][0] % grid[0][1], peak // (grid[0][0] * grid[0][1])]
            assert F4(float(f[8])) == p and p == cluster_p([len(member)], rows[:, c, 2])[0]
            assert (res["cluster_p"][c].reshape(-1)[member] == p).all()
        assert (res["cluster_p"][c][labels == 0] == 1).all()


def test_two_sided_takes_the_larger_side(tool_dir):
    d = tool_dir
    r = run(tool_command(d, "two", "-ct", str(TOOL_T0), "-two", "1"), d)
    assert r.returncode == 0, r.stdout + r.stderr
    grid, two = python_result(d, cluster_threshold=TOOL_T0, two_sided=True)
    _, pos = python_result(d, cluster_threshold=TOOL_T0)
    _, neg = python_result(d, cons=[[0.0, -1.0, 0.0], [0.0, 0.0, -1.0]], cluster_threshold=TOOL_T0)      # -t, to the bit
    assert same(two["max_extent"], np.maximum(pos["max_extent"], neg["max_extent"]))
    assert (pos["max_extent"] != neg["max_extent"]).any()
    rows = np.loadtxt(d / "two" / "maxextent.csv", delimiter=",", skiprows=1).reshape(TOOL_PERMS, 2, 3)
    assert (rows[:, :, 2] == two["max_extent"]).all()
    for c in range(2):
        labels = read_volume(d / "two" / f"clusters_{c}.nii.gz")[0]
        assert same(labels, two["clusters"][c])
        assert same(read_volume(d / "two" / f"cluster_p_{c}.nii.gz")[0], two["cluster_p"][c])
        # the negative side's clusters are numbered after the positive side's
        k = int(pos["clusters"][c].max())
        assert same(np.where(labels <= k, labels, 0), pos["clusters"][c])
        assert same(np.where(labels > k, labels - k, 0).astype(np.int32), neg["clusters"][c])
    signs = [line.split(",")[2] for line in (d / "two" / "clusters.csv").read_text().splitlines()[1:]]
    assert signs.count("1") == sum(int(pos["clusters"][c].max()) for c in range(2)) and signs.count("-1") == sum(int(neg["clusters"][c].max()) for c in range(2))


def test_group_stats_refuses_bad_cluster_options(tool_dir):
    d = tool_dir
    tool = [os.path.join(BIN, "GroupStats"), "bbox.json", SPACING, "design.csv"]
    for k, extra in enumerate((["-ct", "2"], ["-cc", "6", "-np", "5"], ["-cc", "6"], ["-np", "5", "-ct", "-1"], ["-np", "5", "-ct", "nan"],
                               ["-np", "5", "-ct", "inf"], ["-np", "5", "-ct", "2", "-cc", "8"])):
        r = run(tool + ["-o", f"bad{k}"] + extra, d)
        assert r.returncode == 1 and "Error : " in r.stdout and not (d / f"bad{k}").exists(), extra
