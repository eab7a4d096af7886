"""The deformable sweeps elect per STEP of a culling list, not per range (k_links.hip.h, k_cull.hip.h): both list
writers mark the steps of 64 listed records that hold an own point twice, a range whose flag is set takes the lane
election in exactly those steps and the plain read-add-write in the others.  Which lanes meet on a point is a property
of the list and both paths perform the same additions in the same order, so every comparison here is `==`."""
import numpy as np
import pytest

from frog_amd import schedule
from frog_amd.image_group import ImageGroup
from frog_amd.pairs import Pairs
from gpu_util import note

pytestmark = pytest.mark.gpu

TILE_POINTS, N_GROUPS, STEP = 256, 8, 64            # ctx.h: points per sweep tile, partner groups, records per sweep step


# ---- the device layout's record order, restated on the host (prep.h) ----------------------------------------------

def _spread3(v):
    v = v.astype(np.uint32) & np.uint32(0x3FF)
    v = (v | (v << np.uint32(16))) & np.uint32(0x030000FF)
    v = (v | (v << np.uint32(8))) & np.uint32(0x0300F00F)
    v = (v | (v << np.uint32(4))) & np.uint32(0x030C30C3)
    v = (v | (v << np.uint32(2))) & np.uint32(0x09249249)
    return v


def morton_order(x):
    """prep.h build_numbering for one image: the old indices of its points in their new (Morton) order, f32 as there."""
    x = np.asarray(x, np.float32)
    mn, mx = x.min(axis=0), x.max(axis=0)
    ext = (mx - mn).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(ext > 0, (x - mn) / ext, np.float32(0)).astype(np.float32)
    u = np.where(u >= 0, u, np.float32(0))
    u = np.minimum(u, np.float32(1))
    q = (u * np.float32(1023.0)).astype(np.uint32)
    key = _spread3(q[:, 0]) | (_spread3(q[:, 1]) << np.uint32(1)) | (_spread3(q[:, 2]) << np.uint32(2))
    return np.argsort(key, kind="stable")


def steps_of_the_full_list(pairs):
    """(steps, steps that hold an own point twice, their (tile, group, step) keys) of a culling list that leaves no
    half-link out: the records of a (tile, partner group) range are partner-image major, then point order (Morton rank
    inside the tile), then the link table's order; a step is 64 consecutive records of a range."""
    po = np.asarray(pairs.point_offset).astype(np.int64)
    rp = np.asarray(pairs.row_ptr).astype(np.int64)
    li = np.asarray(pairs.link_image).astype(np.int64)
    xyz = np.asarray(pairs.xyz, np.float32).reshape(-1, 3)
    n_img, P = len(po) - 1, int(po[-1])
    new_of_old = np.empty(P, np.int64)
    for i in range(n_img):
        order = morton_order(xyz[po[i]:po[i + 1]])
        new_of_old[po[i] + order] = po[i] + np.arange(len(order))
    group_begin = [0] + [int(np.searchsorted(po[:n_img], P * g // N_GROUPS, "left")) for g in range(1, N_GROUPS)] + [n_img]
    group_of = np.zeros(n_img, np.int64)
    for g in range(N_GROUPS):
        group_of[group_begin[g]:group_begin[g + 1]] = g
    owner = np.repeat(np.arange(P), np.diff(rp))                         # old index of every half-link's own point
    image = np.searchsorted(po, owner, "right") - 1
    local = new_of_old[owner] - po[image]
    tiles_before = np.concatenate([[0], np.cumsum((np.diff(po) + TILE_POINTS - 1) // TILE_POINTS)])
    tile = tiles_before[image] + local // TILE_POINTS
    rank = local % TILE_POINTS
    order = np.lexsort((np.arange(len(li)), rank, li, tile))
    rng = (tile * N_GROUPS + group_of[li])[order]                        # ascending: a group is a run of partner images
    rank = rank[order]
    first = np.concatenate([[True], rng[1:] != rng[:-1]])
    start = np.maximum.accumulate(np.where(first, np.arange(len(rng)), 0))
    step = (np.arange(len(rng)) - start) // STEP
    step_key = rng * (1 << 20) + step
    n_steps = len(np.unique(step_key))
    full_key, count = np.unique(step_key * TILE_POINTS + rank, return_counts=True)
    dup_keys = np.unique(full_key[count > 1] // TILE_POINTS)
    return n_steps, len(dup_keys), [(int(k >> 20) // N_GROUPS, int(k >> 20) % N_GROUPS, int(k & ((1 << 20) - 1))) for k in dup_keys]


# ---- runs -----------------------------------------------------------------------------------------------------------

def _env(monkeypatch, cull, build_pass=False, skin=None):
    monkeypatch.setenv("FROG_CULL", "1" if cull else "0")
    if build_pass:
        monkeypatch.setenv("FROG_CULL_BUILD_PASS", "1")
    else:
        monkeypatch.delenv("FROG_CULL_BUILD_PASS", raising=False)
    if skin:
        monkeypatch.setenv("FROG_CULL_SKIN", skin)
    else:
        monkeypatch.delenv("FROG_CULL_SKIN", raising=False)


def _state(g, pairs):
    return dict(lattices=[[g.grid(i, k)[1].copy() for k in range(g.num_grids())] for i in range(pairs.n_images)],
                sums=g.point_sums().copy(), census=[(c.inliers, c.outliers) for c in g.countInliers()],
                xyz=g.points()[0].copy(), xyz2=g.points()[1].copy())


def _same_state(a, b):
    assert np.array_equal(a["sums"], b["sums"]) and a["census"] == b["census"]
    assert np.array_equal(a["xyz"], b["xyz"]) and np.array_equal(a["xyz2"], b["xyz2"])
    assert len(a["lattices"]) == len(b["lattices"])
    for la, lb in zip(a["lattices"], b["lattices"]):
        assert len(la) == len(lb)
        for x, y in zip(la, lb):
            assert np.array_equal(x, y)


def _run(pairs, linear, levels, iterations, on=None):
    g = ImageGroup(pairs)
    g.linearIterations, g.deformableLevels, g.deformableIterations = linear, levels, iterations
    if on is None:
        E = g.run()
    else:
        E = []

        def hook(tag, sides, e=None, infos=None):
            if schedule.kind(tag) in ("linear", "deformable"):
                E.append(float(np.float32(e[0])))
            on(tag, sides[0])
        g.gridsPerLevel = schedule.run([g], linear, [iterations] * levels, g.statIntervalUpdate, g.deformableAlpha, hook)
    return g, E, _state(g, pairs)


def _steps_directly(pairs, n_steps, alpha=0.02):
    """No linear stage, one lattice, `n_steps` deformable steps: the first walks every record (and writes the list, when
    there is one), the others walk the list.  Returns the group, the energies and the per-point sums after each step."""
    g = ImageGroup(pairs)
    g.setupLinearTransforms(); g.transformPoints(); g.transformPoints(True)
    g.setupDeformableTransforms(0); g.transformPoints(); g.updateStats()
    # distances of some hundredths of a millimetre make degenerate mixtures, which have no certified cutoff and whose
    # list does not outlive a transform: an ordinary mixture instead (every weight is 1 whatever the mixture: d < 0.1)
    for i in range(pairs.n_images):
        g.set_em(i, np.float32([3.0, 200.0, 0.7]))
    E, sums = [], []
    for _ in range(n_steps):
        E.append(g.updateDeformableTransforms(alpha))
        sums.append(g.point_sums().copy())
        g.transformPoints()
    return g, E, sums, _state(g, pairs)


# ---- 1 --------------------------------------------------------------------------------------------------------------

def test_both_list_writers_mark_the_same_steps_and_the_runs_keep_their_bits(monkeypatch):
    """A group of many small images (a step spans several partner images: ranges with and without duplicate steps), 20
    linear + 3 x 25 deformable iterations: without culling, with the list written by the sweep, with the list written by
    the build pass.  Same bits everywhere; the two writers' lists, flags and step bits are the same; some listed steps
    elect, not all, and at least one per flagged range."""
    pairs = Pairs.synthetic(24, 400, 150, seed=5)
    _env(monkeypatch, False)
    g0, E0, S0 = _run(pairs, 20, 3, 25)
    _env(monkeypatch, True)
    g1, E1, S1 = _run(pairs, 20, 3, 25)
    _env(monkeypatch, True, build_pass=True)
    g2, E2, S2 = _run(pairs, 20, 3, 25)
    assert g0.gridsPerLevel == g1.gridsPerLevel == g2.gridsPerLevel
    assert E0 == E1 == E2
    _same_state(S0, S1); _same_state(S0, S2)
    assert g0.cull_stats()[0] == 0 and g0.cull_steps() == (0, 0)
    assert g1.cull_stats() == g2.cull_stats() and g1.cull_stats()[0] >= 1
    assert g1.cull_ranges() == g2.cull_ranges()
    assert g1.cull_steps() == g2.cull_steps()
    (ranges, elected_ranges), (steps, elected_steps) = g1.cull_ranges(), g1.cull_steps()
    note("step_election_many_small_images", f"ranges {ranges}, with election {elected_ranges}; steps {steps}, with election {elected_steps}")
    assert 0 < elected_steps < steps
    assert elected_steps >= elected_ranges


# ---- 2 --------------------------------------------------------------------------------------------------------------

def _duplicates_in_the_middle():
    """Image 0: 700 points.  Every point has ONE link into image 1, except the points of Morton ranks 64..127 of each
    tile, which have THREE: a tile's range is a step of 64 different points, three steps in which all 64 lanes carry
    duplicates, and certified steps again.  Every linked pair is closer than 0.1 mm: weight exactly 1 (stats.h:87), so
    the f32 sums depend on the order of the adds alone, and no half-link is ever left out of a list."""
    rng = np.random.default_rng(21)
    n = 700
    a = rng.uniform(0, 200, (n, 3)).astype(np.float32)
    rank = np.empty(n, np.int64)
    rank[morton_order(a)] = np.arange(n)
    mult = np.where((rank % TILE_POINTS >= 64) & (rank % TILE_POINTS < 128), 3, 1)
    m = int(mult.sum())
    b = (np.repeat(a, mult, axis=0) + rng.uniform(-0.025, 0.025, (m, 3))).astype(np.float32)
    return Pairs.from_arrays([0, n, n + m], np.concatenate([a, b]),
                             [(0, 1, np.repeat(np.arange(n), mult).astype(np.uint32), np.arange(m, dtype=np.uint32))])


def test_steps_in_which_every_lane_is_a_duplicate_inside_a_certified_range(monkeypatch):
    pairs = _duplicates_in_the_middle()
    n_steps, n_dup, where = steps_of_the_full_list(pairs)
    # the construction, checked on the host: steps 1, 2, 3 of image 0's three tiles (all into partner group 3), nothing else
    assert sorted(where) == [(t, 3, s) for t in range(3) for s in (1, 2, 3)], where
    _env(monkeypatch, False)
    g0, E0, sums0, S0 = _steps_directly(pairs, 4)
    _env(monkeypatch, True)
    g1, E1, sums1, S1 = _steps_directly(pairs, 4)
    assert E0 == E1
    for x, y in zip(sums0, sums1):
        assert np.array_equal(x, y)
    _same_state(S0, S1)
    built, listed, owned = g1.cull_stats()
    assert built == 1 and listed == owned == pairs.n_half_links          # one list, used by steps 2..4, nothing left out
    assert g1.cull_steps() == (n_steps, n_dup)
    assert g1.cull_ranges()[1] == 3
    # every point of image 0 was added to as often as it has links: no add lost or doubled
    po, rp = np.asarray(pairs.point_offset), np.asarray(pairs.row_ptr)
    assert np.array_equal(sums1[-1][:, 3], np.diff(rp).astype(np.float32))
    assert po[1] == 700


# ---- 3 --------------------------------------------------------------------------------------------------------------

def _long_ranges():
    """144 images of 256 points (one tile each; partner groups of 18 images), every pair of images linked point by point:
    a (tile, group) range lists 18 x 256 = 4608 records, 72 steps -- more than the 64 steps whose bits a wavefront keeps.
    Points 2k and 2k + 1 coincide for a few k and are linked crosswise into the first and the last image of some groups:
    duplicate steps before and after step 64.  Every linked pair is closer than 0.1 mm, as above."""
    rng = np.random.default_rng(33)
    n_img, n = 144, TILE_POINTS
    base = rng.uniform(0, 200, (n, 3)).astype(np.float32)
    twins = np.array([10, 77, 130, 201])
    base[twins + 1] = base[twins]
    xyz = np.concatenate([(base + rng.uniform(-0.02, 0.02, (n, 3))).astype(np.float32) for _ in range(n_img)])
    p = np.arange(n, dtype=np.uint32)
    blocks = []
    for i in range(n_img):
        for j in range(i + 1, n_img):
            if (i % 18 in (0, 5)) and (j % 18 in (0, 17)):
                k = twins[(i + j) % len(twins)]
                blocks.append((i, j, np.append(p, k).astype(np.uint32), np.append(p, k + 1).astype(np.uint32)))
            else:
                blocks.append((i, j, p, p))
    return Pairs.from_arrays(np.arange(n_img + 1) * n, xyz, blocks)


def test_a_range_longer_than_the_step_window(monkeypatch):
    pairs = _long_ranges()
    n_steps, n_dup, where = steps_of_the_full_list(pairs)
    per_range = {}
    for t, g, s in where:
        per_range.setdefault((t, g), []).append(s)
    assert any(min(s) < 64 <= max(s) for s in per_range.values()), "no range with duplicate steps on both sides of step 64"
    assert any(max(s) < 64 for s in per_range.values()) and any(min(s) >= 64 for s in per_range.values())
    _env(monkeypatch, False)
    g0, E0, sums0, S0 = _steps_directly(pairs, 3)
    _env(monkeypatch, True)
    g1, E1, sums1, S1 = _steps_directly(pairs, 3)
    assert E0 == E1
    for x, y in zip(sums0, sums1):
        assert np.array_equal(x, y)
    _same_state(S0, S1)
    built, listed, owned = g1.cull_stats()
    assert built == 1 and listed == owned == pairs.n_half_links
    assert g1.cull_steps() == (n_steps, n_dup)
    assert g1.cull_ranges()[1] == len(per_range)
    note("step_election_long_ranges", f"steps {n_steps}, with election {n_dup}, in {len(per_range)} ranges")


# ---- 4 --------------------------------------------------------------------------------------------------------------

def test_a_rebuilt_list_does_not_inherit_step_bits(small_pairs, monkeypatch):
    """A thin skin: several lists per run, the later ones shorter.  The run equals the unculled run, and the step bits
    after the last build are those of a fresh context that builds its first list from the same coordinates and mixtures
    (set from outside)."""
    _env(monkeypatch, False)
    g0, E0, S0 = _run(small_pairs, 20, 3, 25)
    _env(monkeypatch, True, skin="1.2,3.0")
    seen = dict(builds=0)

    def on(tag, g):
        if schedule.kind(tag) != "step":
            return
        built, listed, _ = g.cull_stats()
        if built > seen["builds"]:          # this step's sweep wrote a list, from the coordinates and mixtures that still stand
            seen.update(builds=built, level=tag[1], listed=listed, xyz2=g.points()[1].copy(),
                        em=[g.em(i).copy() for i in range(small_pairs.n_images)], steps=g.cull_steps(), ranges=g.cull_ranges())
            seen.setdefault("history", []).append(listed)
    g1, E1, S1 = _run(small_pairs, 20, 3, 25, on=on)
    assert g0.gridsPerLevel == g1.gridsPerLevel and E0 == E1
    _same_state(S0, S1)
    assert seen["builds"] >= 2 and g1.cull_stats()[0] == seen["builds"]
    assert min(seen["history"][1:]) < seen["history"][0]                  # a later list is shorter than the first
    assert g1.cull_steps() == seen["steps"]                               # nothing has touched the bits since

    g2 = ImageGroup(small_pairs)
    schedule.run([g2], 20, [])
    g2.setupDeformableTransforms(seen["level"]); g2.transformPoints()
    for i, em in enumerate(seen["em"]):
        g2.set_em(i, em)
    g2.set_points2(seen["xyz2"])
    g2.updateDeformableTransforms(0.0)
    assert g2.cull_stats()[:2] == (1, seen["listed"])
    assert g2.cull_ranges() == seen["ranges"]
    assert g2.cull_steps() == seen["steps"]
    assert 0 < seen["steps"][1] < seen["steps"][0]
