"""The three half-link sweeps (k_links.hip.h: linear, deformable, counting) and the layout that feeds them (prep.h, k_cull.hip.h)
on the designed links of tests/links_design.py: every half-link weighs exactly 1 or exactly +0 and every sum is exact, so the
per-point sums, both energies, the census, the matrices after one linear step and the length of a culling list are compared
with an order-free f64 restatement bit for bit -- in every form of the sweep, each in contexts of its own, for coordinate
sets A and then B (handed in through set_points2: no sum, count or list survives from A).  A dropped, doubled or mis-attributed
half-link changes an integer at one point, and the failure names it: form, image, index in its tile, degree, group.

Recorded through gpu_util.note per group: the half-links, the near / far split, the listed count, the ranges with election.
"""
import ctypes as C

import numpy as np
import pytest

import links_design as lk
from frog_amd import _abi
from frog_amd.image_group import ImageGroup
from gpu_util import note
from test_gpu_step_election import morton_order       # prep.h build_numbering for one image, restated

pytestmark = pytest.mark.gpu
F = np.float32

SWITCHES = ("FROG_CULL", "FROG_CULL_BUILD_PASS", "FROG_CULL_LINEAR", "FROG_CULL_SKIN", "FROG_CULL_SKIN_LINEAR", "FROG_SWEEP_FUSED",
            "FROG_WIDE_RECORDS", "FROG_SUBPASSES", "FROG_TILE_SLICES", "FROG_WEIGHT_EXACT", "FROG_WEIGHT_GENERAL", "FROG_ENERGY_PASS",
            "FROG_SCALARS_COPY", "FROG_REFERENCE_ORDER", "FROG_REF_LITERAL")
# one switch at a time (switches.h; read at frog_create); "sub_range": contexts that own a middle subset of the images
FORMS = {
    "default": {},
    "cull0": {"FROG_CULL": "0"},
    "build_pass": {"FROG_CULL_BUILD_PASS": "1"},
    "cull_linear0": {"FROG_CULL_LINEAR": "0"},
    "fused0": {"FROG_SWEEP_FUSED": "0"},
    "fused1": {"FROG_SWEEP_FUSED": "1"},
    "wide": {"FROG_WIDE_RECORDS": "1"},
    "subpasses2": {"FROG_SUBPASSES": "2"},
    "subpasses8": {"FROG_SUBPASSES": "8"},
    "slices1": {"FROG_TILE_SLICES": "1"},
    "slices3": {"FROG_TILE_SLICES": "3"},
    "weight_exact": {"FROG_WEIGHT_EXACT": "1"},
    "weight_general": {"FROG_WEIGHT_GENERAL": "1"},
    "energy_pass": {"FROG_ENERGY_PASS": "1"},
    "scalars_copy": {"FROG_SCALARS_COPY": "1"},
    "reference_order": {"FROG_REFERENCE_ORDER": "1"},
    "sub_range": {},
}
NO_LIST = ("cull0", "reference_order")              # forms whose deformable sweeps walk every record, always
# the images a "sub_range" context owns: its first point is not point 0, and the images before and behind it have links into it
SUB_RANGE = {"g3": (1, 2), "g9": (2, 7), "g24": (7, 20), "g300": (100, 200)}


def set_switches(monkeypatch, env):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


_expected = {}


def expected(name, which):
    """The restatement of group `name` at coordinate set `which`, computed once and left unchanged."""
    if (name, which) not in _expected:
        g = lk.build(name)
        _expected[(name, which)] = (lk.expected(g, g.coordinates(which)), lk.half_links(g, g.coordinates(which)))
    return _expected[(name, which)]


def _tile_rank(g, point):
    """(tile of its image, index in the tile) of a point in the device's numbering (prep.h build_numbering)."""
    i = g.image_of(point)
    order = morton_order(g.xyz[g.po[i]:g.po[i + 1]])
    rank = int(np.nonzero(order == point - g.po[i])[0][0])
    return rank // lk.TILE_POINTS, rank % lk.TILE_POINTS


def check_sums(g, got, want, rows, tag):
    lo, hi = rows
    bad = np.nonzero(np.any(got[lo:hi].view(np.uint32) != want["sums"][lo:hi].view(np.uint32), axis=1))[0]
    if len(bad):
        p = int(lo + bad[0])
        i = g.image_of(p)
        tile, rank = _tile_rank(g, p)
        pytest.fail(f"{g.name} {tag}: {len(bad)} points differ; first: point {p} = image {i} (partner group {int(g.group_of[i])}), tile {tile}, "
                    f"index {rank} in the tile, degree {int(want['degree'][p])}: got {got[p].tolist()}, expected {want['sums'][p].tolist()}")


def check_margins(h, cut_list, tag):
    """No far distance within a factor 1.01 of the cutoff that decides about it: the list's length does not hang on a rounding."""
    cut = np.minimum(np.asarray(cut_list, np.float64)[h["image"]], np.asarray(cut_list, np.float64)[h["image_other"]])
    d = np.sqrt(h["d2"])
    assert not np.any((d > cut / 1.01) & (d < cut * 1.01)), tag


def listed_of(g, h, cut_list, images):
    cut = np.asarray(cut_list, F)
    keep = lk.listed(h["d2_f32"], cut[h["image"]], cut[h["image_other"]])
    return int(np.count_nonzero(keep & (h["image"] >= images[0]) & (h["image"] < images[1])))


def energy_of(want, d2, n, images):
    with np.errstate(all="ignore"):
        return float(np.sqrt(want[d2][images[0]:images[1]].sum() / want[n][images[0]:images[1]].sum()))


class Context:
    """An ImageGroup over the whole group or over an image range, behind the verbs both kinds have."""

    def __init__(self, name, image_range=None):
        self.group = lk.build(name)
        self.whole = image_range is None
        self.images = image_range or (0, self.group.n_images)
        self.g = ImageGroup(lk.pairs(name), image_range=image_range)
        self.lib = self.g._lib

    def transform(self, apply=False):
        if self.whole:
            self.g.transformPoints(apply)
        else:
            _abi.check(self.lib.frog_transform_points_local(self.g._ctx, int(apply)), "frog_transform_points_local")

    def lattice(self):
        if self.whole:
            self.g.setupDeformableTransforms(0)
        else:
            self.g.deformable_setup_bounds(0, [0.0] * 3, [64.0] * 3)

    def linear_step(self):
        if self.whole:
            return self.g.updateLinearTransforms()
        e = C.c_double()
        _abi.check(self.lib.frog_linear_step_local(self.g._ctx), "frog_linear_step_local")
        _abi.check(self.lib.frog_energy_read(self.g._ctx, C.byref(e), None), "frog_energy_read")
        return e.value

    def deformable_step(self):
        if self.whole:
            return self.g.updateDeformableTransforms(0.0)
        e = C.c_double()
        _abi.check(self.lib.frog_deformable_phase_a(self.g._ctx, C.c_float(0.0)), "frog_deformable_phase_a")
        _abi.check(self.lib.frog_deformable_phase_b(self.g._ctx), "frog_deformable_phase_b")
        _abi.check(self.lib.frog_deformable_phase_c(self.g._ctx, C.byref(e)), "frog_deformable_phase_c")
        return e.value


def linear_stage(name, form, which, image_range=None):
    """One linear step at coordinate set `which` on a context used for nothing else (the step starts from the linear
    initialisation): E, every owned image's scale and translation, the length of the linear stage's list where there is one.
    Returns (lists built, listed)."""
    c = Context(name, image_range)
    g, dev, images = c.group, c.g, c.images
    want, h = expected(name, which)
    dev.setupLinearTransforms(); c.transform()
    dev.set_em_rows(g.em_table())
    dev.set_points2(g.coordinates(which))
    start = np.eye(4)
    start[:3, 3] = want["t0"]
    for i in range(*images):
        assert np.array_equal(dev.matrix(i), start), (name, form, which, i)
    e = c.linear_step()
    assert e == energy_of(want, "l_d2", "l_n", images), (name, form, which, e)
    for i in range(*images):
        m = dev.matrix(i)
        assert np.array_equal(np.diag(m)[:3], want["scale"][i], equal_nan=True), (name, form, which, i, np.diag(m)[:3], want["scale"][i], want["power"][i])
        assert np.array_equal(m[:3, 3], want["translation"][i], equal_nan=True), (name, form, which, i, m[:3, 3], want["translation"][i])
    built, listed, owned = dev.cull_stats_linear()
    assert owned == int(np.count_nonzero((h["image"] >= images[0]) & (h["image"] < images[1])))
    if built:
        cut_list = dev.cull_readback()["cut_list"]
        check_margins(h, cut_list, (name, form, which, "linear"))
        assert (built, listed) == (1, listed_of(g, h, cut_list, images)), (name, form, which)
        assert listed == int(want["e_n"][images[0]:images[1]].sum())     # every far link is beyond the linear list's cutoff
    dev.close()
    return built, listed


def deformable_stage(name, form, image_range=None):
    """Coordinate set A: two steps at alpha 0 (the first walks every record and writes the list, or sweeps the list a pass of its
    own wrote; the second walks the list).  Then set B through set_points2: three steps (the list of A is stale: every record;
    the list is rebuilt; the new list is walked).  After every step the per-point sums and the energy, after each set the
    census, after each build the list's length.  Returns what the notes record."""
    c = Context(name, image_range)
    g, dev, images = c.group, c.g, c.images
    rows = (int(g.po[images[0]]), int(g.po[images[1]]))
    has_list = form not in NO_LIST
    dev.setupLinearTransforms(); c.transform(); c.transform(True)
    c.lattice(); c.transform()
    dev.set_em_rows(g.em_table())
    out = {}
    builds = 0
    for which, steps, build_at in (("A", 2, 0), ("B", 3, 1)):
        want, h = expected(name, which)
        assert want["other"] == 0
        dev.set_points2(g.coordinates(which))
        for step in range(steps):
            tag = f"form {form}, set {which}, step {step}"
            e = c.deformable_step()
            check_sums(g, dev.point_sums(), want, rows, tag)
            assert e == energy_of(want, "e_d2", "e_n", images), (name, tag, e)
            if has_list and step == build_at:
                builds += 1
                cut_list = dev.cull_readback()["cut_list"]
                check_margins(h, cut_list, (name, tag))
                n_listed = listed_of(g, h, cut_list, images)
                assert n_listed < len(h["own"]) or not c.whole
                built, listed, owned = dev.cull_stats()
                assert (built, listed) == (builds, n_listed), (name, tag, built, listed, builds, n_listed)
                ranges, elect = dev.cull_ranges()
                list_steps, elect_steps = dev.cull_steps()
                assert elect < ranges and elect <= elect_steps < list_steps, (name, tag, ranges, elect, list_steps, elect_steps)
                assert elect > 0 or not c.whole, (name, tag)
                if name == "g3" and (c.whole or images[0] == 0):
                    # the hub's 1000 and the duplicate's 300 records are runs of one own point: 14 and 3 steps hold nothing else
                    assert elect_steps >= 17, (name, tag, elect_steps)
                out[which] = dict(listed=listed, ranges=ranges, elect=elect, steps=list_steps, elect_steps=elect_steps)
            assert dev.cull_stats()[0] == (builds if has_list else 0), (name, tag)
        counts = dev.countInliers()
        for i in range(*images):
            assert (int(counts[i].inliers), int(counts[i].outliers)) == (int(want["inliers"][i]), int(want["outliers"][i])), (name, form, which, i)
            assert int(counts[i].pairs) == int(want["inliers"][i] + want["outliers"][i]) and int(counts[i].points) == int(g.po[i + 1] - g.po[i])
    dev.close()
    return out


def forms_of(name):
    return ("default", "cull0") if name == "g2100" else tuple(FORMS)


@pytest.mark.parametrize("name", lk.GROUPS)
def test_the_linear_sweep_on_designed_links(monkeypatch, name):
    """One linear step from the linear initialisation, per form and for coordinate sets A then B, each in a context of its own:
    E == sqrt(sum fl32(fl32(sqrt d2)^2) / sum 1) over the near half-links, every image's scale and translation ==
    linear_update_kernel's formula on the exact sums (an image without a near link keeps its matrix: 0 / 0), the linear list
    holds exactly the near half-links."""
    g = lk.build(name)
    assert not np.array_equal(expected(name, "A")[0]["linear_sums"], expected(name, "B")[0]["linear_sums"])
    for which in "AB":
        lists = {}
        for form in forms_of(name):
            set_switches(monkeypatch, FORMS[form])
            lists[form] = linear_stage(name, form, which, SUB_RANGE[name] if form == "sub_range" else None)
        want, _ = expected(name, which)
        assert lists["default"] == (1, want["near"])
        assert lists["cull0"][0] == 0
        if name != "g2100":
            assert lists["cull_linear0"][0] == 0 and lists["weight_exact"][0] == 0 and lists["build_pass"] == lists["default"]
        note(f"links_design_{name}_linear_{which}", f"half-links {g.n_half_links}, near {want['near']}, far {want['far']}, in the linear list {lists['default'][1]}")


@pytest.mark.parametrize("name", lk.GROUPS)
def test_the_deformable_and_counting_sweeps_on_designed_links(monkeypatch, name):
    """Per form, coordinate sets A then B: per-point sums == the sum of (partner - own) over the point's near half-links and
    their number, at every point (exact zeros at unlinked and far-only points), after the walk of every record, after the walk of
    the list, after the stale list and after the rebuilt one; E == sqrt(sum d2 / sum 1); the census per image; the list's length
    == the half-links below min of the two images' list cutoffs as read back."""
    g = lk.build(name)
    for which in "AB":                                      # the two sets ask for different sums at the moved image's points
        assert expected(name, which)[0]["other"] == 0
    assert not np.array_equal(expected(name, "A")[0]["sums"], expected(name, "B")[0]["sums"])
    seen = {}
    for form in forms_of(name):
        set_switches(monkeypatch, FORMS[form])
        seen[form] = deformable_stage(name, form, SUB_RANGE[name] if form == "sub_range" else None)
    d = seen["default"]
    wa, wb = expected(name, "A")[0], expected(name, "B")[0]
    for form, s in seen.items():                            # which steps hold a point twice is a property of the list
        if form not in NO_LIST + ("sub_range", "subpasses2", "subpasses8"):
            assert s == d, (name, form, s, d)
    note(f"links_design_{name}", f"half-links {g.n_half_links}; set A: near {wa['near']} far {wa['far']} listed {d['A']['listed']}, ranges {d['A']['ranges']} "
                                 f"with election {d['A']['elect']}, steps {d['A']['steps']} with election {d['A']['elect_steps']}; set B: near {wb['near']} "
                                 f"far {wb['far']} listed {d['B']['listed']}, ranges {d['B']['ranges']} with election {d['B']['elect']}")
