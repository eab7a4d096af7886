"""The designed links of tests/links_design.py on the CPU: the classes are there, the conditions the exactness rests on hold,
and the oracle -- the reference's arithmetic, in the reference's order -- equals the order-free f64 restatement with `==`: the
per-point sums, the energy and the census of a deformable step, the energy of a linear step and every image's scale and
translation after it, for both coordinate sets of every group.  The same comparisons run on the device, in every form of the
sweep, in tests/test_gpu_links_design.py."""
import numpy as np
import pytest

import cull_restate as cr
import links_design as lk
from frog_amd import _abi
from oracle.oracle_api import OracleGroup

F = np.float32


def test_the_designed_classes_are_there():
    c = {name: lk.classes(lk.build(name)) for name in lk.GROUPS}
    for name, k in c.items():
        print(name, k)
    # tiles of 2, 3, 255, 256 and 257 = 256 + 1 points; an image of two full tiles; images of many tiles
    assert {2, 3, 255, 256, 1} <= c["g9"]["tiles"]
    assert sorted(int(n) for n in np.diff(lk.build("g9").po)) == sorted(n + 2 for n in lk.G9_EXTRAS) and {0, 1, 253, 254, 255} <= set(lk.G9_EXTRAS)
    assert int(np.diff(lk.build("g3").po)[2]) == 2 * lk.TILE_POINTS and c["g3"]["tiles_per_image_max"] >= 12
    # image counts and what they do to the partner groups
    assert [c[n]["images"] for n in lk.GROUPS] == [3, 9, 24, 300, 2100]
    assert c["g3"]["empty_groups"] == 5
    assert c["g9"]["empty_groups"] == 0 and c["g24"]["empty_groups"] == 0 and c["g24"]["widest_group"] == 3
    assert 24 <= c["g300"]["widest_group"] <= 64
    assert c["g2100"]["widest_group"] > 256 and c["g2100"]["tiles"] <= {3, 4}
    # range lengths per (tile, partner group): g24's images are one tile each
    assert set(lk.RANGE_LENGTHS) | {0} <= c["g24"]["range_lengths"]
    assert {1, 63, 64, 65, 127, 128, 129, 383, 384, 385} <= set(lk.RANGE_LENGTHS) and max(lk.RANGE_LENGTHS) > lk.STEP * lk.STEP_WINDOW
    assert (lk.STEP, lk.REC_CHUNK, lk.BODY_STEPS * lk.STEP) == (64, 128, 384)
    total, _, _ = lk.range_lengths(lk.build("g24"))
    for i, want in enumerate(lk.RANGE_LENGTHS):             # image i: that many records into group 4 + i // 3, and no other
        row = total[i].copy()
        assert row[4 + i // 3] == want, (i, row)
        row[4 + i // 3] = 0
        assert row.sum() == (1 if i % 3 == 0 else 0), (i, row)      # the first image of a group has its zero record
    assert not total[11].any()
    assert c["g24"]["ranges_near_only"] >= 1 and c["g24"]["ranges_far_only"] >= 1 and c["g24"]["ranges_mixed"] >= 1
    # degrees
    g3, e3 = lk.build("g3"), lk.expected(lk.build("g3"), lk.build("g3").xyz)
    deg, cnt = e3["degree"], e3["sums"][:, 3]
    m = g3.marks
    assert deg[m["no_link"]] == 0 and deg[m["far_only"]] > 0 and cnt[m["far_only"]] == 0
    assert deg[m["degree1"]] == 1 and deg[m["degree2"]] == 2 and deg[m["degree64"]] == 64 and deg[m["degree65"]] == 65
    assert deg[m["duplicate300"]] == 300 and c["g3"]["max_multiplicity"] == 300
    assert deg[m["hub"]] == 1000 and cnt[m["hub"]] == 1000 and c["g3"]["max_distinct_near_partners"] == 1000
    for name in lk.GROUPS:
        k = c[name]
        assert k["unlinked"] >= 1 and k["far_only"] >= 1 and {0, 1, 2} <= k["degrees"], name
        # the all-zero record, one per non-empty group, both directions
        assert k["zero_record_groups"] == k["non_empty_groups"] and k["zero_records"] >= k["non_empty_groups"], name
        assert k["far"] > 0 and k["near"] > 0 and k["far_min"] >= lk.FAR_D
    assert {64, 65, 300, 1000} <= c["g3"]["degrees"]
    # far distances: inside the list's skin, beyond it, beyond 100 -- none within 2 % of the list cutoff as restated (the device
    # test checks 1 % against the cutoffs it reads back)
    for name in ("g3", "g9", "g300"):
        assert c[name]["far_31"] > 0 and c[name]["far_40"] > 0 and c[name]["far_100"] > 0, name
    assert c["g2100"]["far_31"] > 0 and c["g2100"]["far_40"] > 0
    cut_now = cr.cull_cutoff_of(lk.EM, 0.5)
    cut_list = float(cr.list_cutoff(cut_now, 2.0, 25.0))
    lin_list = float(cr.list_cutoff(cr.cull_cutoff_linear_of(lk.EM), 1.25, 10.0))
    assert 4.0 < cut_now < 5.0 and 33.0 < cut_list < 35.0 and lin_list < lk.FAR_D / 1.02
    for name in lk.GROUPS:
        g = lk.build(name)
        for which in "AB":
            h = lk.half_links(g, g.coordinates(which))
            d = np.sqrt(h["d2"][h["d2"] > lk.NEAR_D2])
            assert not np.any((d > cut_list / 1.02) & (d < cut_list * 1.02)), (name, which)
            assert np.any(d < cut_list) and np.any(d > cut_list)


@pytest.mark.parametrize("name", lk.GROUPS)
def test_the_conditions_exactness_rests_on(name):
    g = lk.build(name)
    ea, eb = lk.expected(g, g.xyz), lk.expected(g, g.xyz_b)
    for which, e in (("A", ea), ("B", eb)):
        x = g.coordinates(which).astype(np.float64)
        assert np.array_equal(x * lk.UNIT, np.round(x * lk.UNIT)) and x.min() >= 0 and x.max() <= 64
        for i in range(g.n_images):
            assert np.array_equal(x[g.po[i]], [0, 0, 0]) and np.array_equal(x[g.po[i] + 1], [64, 64, 64])
        h = lk.half_links(g, g.coordinates(which))
        near = h["d2"] <= lk.NEAR_D2
        assert np.all(np.sqrt(h["d2"][~near]) >= lk.FAR_D) and e["other"] == 0          # near d2 <= 0.0029, far d >= 30, no other link
        assert np.all(h["d2_f32"][near] < F(0.01)) and lk.NEAR_D2 < 0.01
        assert e["near"] + e["far"] == g.n_half_links and e["near"] > 0 and e["far"] > 0
        assert e["variance_bits"] <= 53                     # sWeight sPos2 and sPos^2: exact in f64
        assert np.abs(e["sums"][:, :3]).max() * lk.UNIT < 2 ** 24 and e["sums"][:, 3].max() < 2 ** 24
        # the scale is fl32(pow(ratio, 0.5 alpha)): the f64 power is farther than 2^-40 relative from the midpoint of two f32
        p = e["power"][np.isfinite(e["power"]) & (e["power"] > 0)]
        assert len(p) > 0
        f = p.astype(F)
        for other in (np.nextafter(f, F(np.inf)), np.nextafter(f, F(0))):
            mid = 0.5 * (f.astype(np.float64) + other.astype(np.float64))
            assert np.all(np.abs(p - mid) > 2.0 ** -40 * p), (name, which)
    # set B: the moved image's near links of A are far and its far links of A near; every other link is what it was
    ha, hb = lk.half_links(g, g.xyz), lk.half_links(g, g.xyz_b)
    of_moved = (ha["image"] == g.moved) | (ha["image_other"] == g.moved)
    frame = (ha["own"] - g.po[ha["image"]] < 2) | (ha["other"] - g.po[ha["image_other"]] < 2)
    near_a, near_b = ha["d2"] <= lk.NEAR_D2, hb["d2"] <= lk.NEAR_D2
    assert np.array_equal(near_a[~of_moved | frame], near_b[~of_moved | frame])
    flips = of_moved & ~frame
    assert np.array_equal(near_a[flips], ~near_b[flips]) and np.any(near_a[flips]) and np.any(near_b[flips])
    assert not np.array_equal(ea["sums"], eb["sums"]) and not np.array_equal(ea["inliers"], eb["inliers"])


def _oracle(g):
    ref = OracleGroup(lk.pairs(g.name).model, _abi.FrogOptions.default())
    ref.setup_stats()
    ref.linear_init(); ref.transform_points()
    start = np.eye(4)
    start[:3, 3] = lk.linear_init_translation(g.n_images)
    assert np.array_equal(ref.xyz(), g.xyz) and abs(start[0, 3]) < 2.0 ** -10
    assert (start[0, 3] == 0 and np.array_equal(ref.xyz2(), g.xyz)) or g.n_images > 9
    for i in range(g.n_images):
        assert np.array_equal(ref.matrix(i), start), i
    return ref


def _set_mixtures(ref, g):
    for i in range(g.n_images):
        ref.set_em(i, F(lk.EM))


@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("name", lk.GROUPS)
def test_the_oracle_equals_the_restatement(name, which):
    g = lk.build(name)
    x2 = g.coordinates(which)
    want = lk.expected(g, x2)
    # the deformable step and the census
    ref = _oracle(g)
    ref.transform_points(True)
    ref.deformable_setup(0, _abi.FrogGridInfo())
    ref.transform_points()
    _set_mixtures(ref, g)
    ref.set_xyz2(x2)
    e = ref.deformable_step(0.0)
    sums = ref.point_sums()
    bad = np.nonzero(np.any(sums != want["sums"], axis=1))[0]
    assert len(bad) == 0, (name, which, len(bad), int(bad[0]), g.image_of(bad[0]), sums[bad[0]], want["sums"][bad[0]])
    if g.marks and which == "A":                            # exact zeros at an unlinked point and at one with far links only
        assert not sums[g.marks["no_link"]].any() and not sums[g.marks["far_only"]].any()
    assert e == want["E"], (e, want["E"])
    counts = ref.count_inliers((_abi.FrogCounts * g.n_images)())
    assert [int(c.inliers) for c in counts] == list(want["inliers"]) and [int(c.outliers) for c in counts] == list(want["outliers"])
    # one linear step from the identity, on an oracle used for nothing else
    ref = _oracle(g)
    _set_mixtures(ref, g)
    ref.set_xyz2(x2)
    e = ref.linear_step()
    assert e == want["E_linear"], (e, want["E_linear"])
    for i in range(g.n_images):
        m = ref.matrix(i)
        assert np.array_equal(np.diag(m)[:3], want["scale"][i], equal_nan=True), (name, which, i, np.diag(m)[:3], want["scale"][i])
        assert np.array_equal(m[:3, 3], want["translation"][i], equal_nan=True), (name, which, i, m[:3, 3], want["translation"][i])
        off = m.copy()
        off[[0, 1, 2], [0, 1, 2]] = 0
        off[:3, 3] = 0
        assert np.array_equal(off, np.diag([0.0, 0, 0, 1]))
    moved = np.count_nonzero(want["scale"] != 1.0)
    assert moved > 0 and np.count_nonzero(want["translation"]) > 0
