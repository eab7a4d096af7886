"""The control-point step -- lattice_step_kernel<true> for a context that owns the group, lattice_step_kernel<false> + the
all-reduce + cp_center_kernel for contexts that own sub-ranges (k_grid.hip.h) -- on the many-image group of
tests/step_design.py, at the image and node counts where the kernels switch paths:

  images   2 .. 577: one pass of LS_IC = 64 images, a full pass, a ragged last pass, the LS_KEEP * LS_IC = 512 owned images
           up to which the proposals wait in registers (511, 512) and beyond which they are stored and re-read (513, 577);
  nodes    3375 (blocks of LS_CPB = 16, the last one partial), 729 < LS_SMALL_NODES (blocks of LS_CPB_SMALL = 4, the last
           one partial) and exactly 2048 (the first lattice of the wide shape);
  slots    bricks of 2, 5, 6 and 11 scatter blocks: one, one full, two and three trips of the four-at-a-time slot loop;
  count    the guard's oversize count, read back and compared with the count over the read-back coefficients at a limit
           placed ON an attained coefficient and one float below it -- dense and sparse, where a node's inactive pairs are
           counted n_inactive at a time;
  shards   owned counts 9, 10, 11, 21 and 14 around cp_center_kernel's batches of CP_BATCH = 10.

Every coefficient of every image is compared with lattice_design.step under its derived bound; the restatement is handed the
run's own per-point sums, coordinates and previous coefficients.  Recorded through gpu_util.note per case: the worst err / bound
and the class of node it sits on.
"""
import ctypes as C

import numpy as np
import pytest

from frog_amd import _abi
from frog_amd.image_group import ImageGroup
from gpu_util import note
import lattice_design as ld
import step_design as sd

pytestmark = pytest.mark.gpu

ALPHA = 1.0
SWITCHES = ("FROG_BRICK", "FROG_LATTICE_BLOCKED", "FROG_LATTICE_SPARSE", "FROG_K11_POINTWISE", "FROG_K11_TILED", "FROG_K11_F64",
            "FROG_ENERGY_PASS", "FROG_REFERENCE_ORDER", "FROG_REF_LITERAL")
FORMS = {
    "default": {},
    "sparse": {"FROG_LATTICE_SPARSE": "1"},
    "blocked": {"FROG_LATTICE_BLOCKED": "1"},
    "blocked_sparse": {"FROG_LATTICE_BLOCKED": "1", "FROG_LATTICE_SPARSE": "1"},
}
PASS_ENDS = (0, 1, 2, 63, 64, 127, 511, 512)        # images named per case beside the worst: the first three, the ends of passes


def start(monkeypatch, n_images, lattice="wide", form="default", **opt):
    """A group at the frame, on its lattice: linear_init .. the lattice's first transform, as ImageGroup::run orders them."""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in FORMS[form].items():
        monkeypatch.setenv(name, value)
    lattice_opt, box = sd.THRESHOLD[:2] if lattice == "threshold" else sd.LATTICES[lattice][:2]
    g = ImageGroup(sd.pairs(n_images), **{**sd.OPTIONS, **lattice_opt, **opt})
    g.setupLinearTransforms(); g.transformPoints(); g.transformPoints(True)
    info = g.setupDeformableTransforms(0) if box is None else g.deformable_setup_bounds(0, *box)
    g.transformPoints(); g.updateStats()
    return g, info


def step_scalars(g):
    """(E, oversize count) of the last step: frog_energy_read copies the context's four step scalars out -- after
    frog_deformable_step they are that step's (the count is zeroed by the next step's energy sums, frog_hip.hip)."""
    e, n = C.c_double(), C.c_double()
    _abi.check(g._lib.frog_energy_read(g._ctx, C.byref(e), C.byref(n)), "frog_energy_read")
    return e.value, n.value


def coefficients(g, n_images, first=0):
    """[images, n_cp, 3] of the newest lattice; the rows of the fixed images (below `first`) are zero: the library keeps no
    lattice for them (fixed_images_have_no_lattice below)."""
    k = g.num_grids() - 1
    rows = [g.grid(i, k)[1] for i in range(first, n_images)]
    return np.concatenate([np.zeros((first,) + rows[0].shape, np.float32), np.stack(rows)])


def limit(ratio, info):
    return [float(np.float32(ratio)) * s for s in info.spacing]      # (double) maxDisplacementRatio * spacing, imageGroup.cxx:425


def take_steps(name, n_images, g, info, steps, lattice, first=0, restate=True):
    """`steps` deformable steps at ALPHA of a group whose guard is off.  Per step: the energy, the per-point sums, no strays and
    -- with `restate` -- every coefficient of every image within 2 x bound of lattice_design.step.  Returns per step a dict of
    the coefficients, the count and E as read back."""
    po, xyz, blocks = sd.build(n_images)
    lat = ld.Lattice.of(info)
    x, x2 = g.points()
    if lattice != "threshold":
        sd.check_frame(info, lattice, x, x2, xyz, n_images, first)
        for image in (0, 1):                                    # the slot counts, from the run's own coordinates and lattice
            sd.check_slots(x[po[image]:po[image + 1]], lat, lattice)
    assert np.array_equal(x2, x) and np.abs(x.astype(np.float64) - xyz).max() <= 2.0 ** -12
    assert not ld.outside(x, lat).any() and g.stray_points() == 0
    n_links = sd.links_per_point(po, blocks).astype(np.float32)
    act = sd.active(lat, po, x)
    arm_at = sd.layout(0, n_images)[0]["arms"]
    arm_nodes = sd.active(lat, np.array([0, po[1] - arm_at]), x[arm_at:po[1]])[0]
    c_prev = coefficients(g, n_images, first)
    assert not c_prev.any()
    out, worst = [], (0.0, "none", -1)
    for it in range(steps):
        x2 = g.points()[1]
        assert sd.link_lengths(po, blocks, x2).max() < 0.095     # every weight is the constant 1
        want_e = ld.energy(po, blocks, x2)[0] if first == 0 else sd.energy(po, blocks, x2, first)
        e = g.updateDeformableTransforms(ALPHA)
        e_read, count = step_scalars(g)
        assert e == e_read and abs(e - want_e) <= 1e-6 * want_e, (name, it, e, e_read, want_e)
        assert g.stray_points() == 0
        c = coefficients(g, n_images, first)
        if restate:
            sums = g.point_sums()
            assert np.array_equal(sums[po[first]:, 3], n_links[po[first]:])      # a point's weight sum: the number of its links
            r = ld.step(lat, po, x, sums, c_prev, ALPHA, mean_over=None if first else ld.ALL_IMAGES, first_image=first)
            assert np.all((r["gw"] == 0) | (r["gw"] >= 2.0 ** -140))             # the condition the bound is derived under
            ratio, at = ld.worst_ratio(r["new"], r["bound"], c)
            where = sd.node_class(act, int(at[1]), arm_nodes)
            ends = {i: round(ld.worst_ratio(r["new"][i], r["bound"][i], c[i])[0], 3) for i in sorted(set(PASS_ENDS + (n_images - 1,))) if first <= i < n_images}
            print(f"{name} step {it}: err / bound {ratio:.3f} in image {at[0]} at node {at[1]} ({where}); by image {ends}; count {count:.0f}")
            assert ratio <= 2.0, (name, it, ratio, at, where)
            if ratio > worst[0]:
                worst = (ratio, where, int(at[0]))
        out.append({"coeffs": c, "count": count, "E": e})
        g.transformPoints()
        c_prev = c
    if restate:
        assert float(np.abs(g.points()[1].astype(np.float64) - x).max()) >= sd.MOVED or steps < 2
        note(f"step_design_{name}", f"worst err/bound {worst[0]:.3f} in image {worst[2]} at {worst[1]}")
    return {"steps": out, "info": info, "x": x, "active": act}


_runs = {}


def run_case(monkeypatch, n_images, lattice, form):
    """Two restated steps of the group in one form; kept for the tests that compare forms and counts with them."""
    key = (n_images, lattice, form)
    if key not in _runs:
        g, info = start(monkeypatch, n_images, lattice, form)
        _runs[key] = take_steps(f"{lattice}_{n_images}_{form}", n_images, g, info, 2, lattice)
        mn, mx = (C.c_double * 3)(), (C.c_double * 3)()
        _abi.check(g._lib.frog_bounds_local(g._ctx, mn, mx), "frog_bounds_local")
        _runs[key]["box"] = (list(mn), list(mx))
        g.close()
    return _runs[key]


# ---- image counts and node counts ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_images", [2, 63, 64, 65, 128, 129, 511, 512, 513, 577])
def test_image_counts_on_the_wide_lattice(monkeypatch, n_images):
    """15^3 nodes, blocks of 16 nodes (the last one partial), the default form.  Up to 512 images the proposals are kept."""
    r = run_case(monkeypatch, n_images, "wide", "default")
    n_cp = int(np.prod(list(r["info"].dims)))
    assert list(r["info"].dims) == [15, 15, 15] and n_cp >= 2048 and n_cp % 16 != 0
    if n_images not in (65, 513):
        del _runs[(n_images, "wide", "default")]                # only these are compared with other runs


@pytest.mark.parametrize("n_images", [2, 65, 513])
def test_image_counts_on_the_narrow_lattice(monkeypatch, n_images):
    """9^3 nodes at spacing 16: below LS_SMALL_NODES, blocks of 4 nodes, the last one partial."""
    r = run_case(monkeypatch, n_images, "narrow", "default")
    n_cp = int(np.prod(list(r["info"].dims)))
    assert list(r["info"].dims) == [9, 9, 9] and n_cp < 2048 and n_cp % 4 != 0
    del _runs[(n_images, "narrow", "default")]


def test_the_first_lattice_of_the_wide_shape(monkeypatch):
    """Exactly LS_SMALL_NODES = 2048 nodes (8 x 16 x 16, a box wider than the points on two axes): the wide block shape, every
    block full.  65 images."""
    g, info = start(monkeypatch, 65, "threshold")
    assert list(info.dims) == sd.THRESHOLD[2] and int(np.prod(list(info.dims))) == 2048
    take_steps("threshold_65_default", 65, g, info, 2, "threshold")
    g.close()


# ---- the layouts among themselves ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_images", [65, 513])
def test_layouts_among_themselves(monkeypatch, n_images):
    """Sparse, blocked and both: the default form's bits in every coefficient over two steps (65 images: kept; 513: stored and
    re-read, lat_active asked again in centre).  In the sparse runs the second step starts from inactive pairs whose shared
    value is not zero -- they took -mean in the first --, so the u_node path carries a value."""
    plain = run_case(monkeypatch, n_images, "wide", "default")
    act = plain["active"]
    assert np.any(~act)
    for form in ("sparse", "blocked", "blocked_sparse"):
        r = run_case(monkeypatch, n_images, "wide", form)
        for it in range(2):
            assert np.array_equal(r["steps"][it]["coeffs"], plain["steps"][it]["coeffs"]), (form, it)
            assert r["steps"][it]["count"] == plain["steps"][it]["count"], (form, it)
        if "sparse" in form:
            c1 = r["steps"][0]["coeffs"]
            lo = np.where(act[:, :, None], np.float32(np.inf), c1).min(axis=0)      # the inactive pairs' values, node by node
            hi = np.where(act[:, :, None], np.float32(-np.inf), c1).max(axis=0)
            some = (~act).any(axis=0)
            assert np.array_equal(lo[some], hi[some])           # one value per node ...
            assert np.count_nonzero(lo[some]) > 100             # ... and not zero: what the second step's u_node reads
        if form != "sparse":                                    # (the count's test starts from the sparse run)
            del _runs[(n_images, "wide", form)]


# ---- the count, exactly and at the limit -----------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["default", "sparse"])
@pytest.mark.parametrize("n_images", [65, 513])
def test_the_count_at_the_limit(monkeypatch, n_images, form):
    """Spacing 8: the limit r * 8 can be put ON an attained |coefficient| v.  A: guard off, read all coefficients.  B: ratio r,
    guard off: A's bits, the count equals the strict count over them (entries equal to v do not count).  C: one float below
    r: more by exactly the entries equal to v.  D: C's ratio, guard on: rejected, nothing changed.  E: a ratio just above
    max |C| / 8, guard on: accepted, A's bits.  Sparse: B's second step too, whose inactive pairs hold -mean of the first."""
    a = run_case(monkeypatch, n_images, "wide", form)
    info = a["info"]
    assert list(info.spacing) == [8.0] * 3
    c1, c2 = a["steps"][0]["coeffs"], a["steps"][1]["coeffs"]
    assert a["steps"][0]["count"] == sd.oversize(c1, limit(sd.OPTIONS.get("max_displacement_ratio", 0.4), info))
    r, v, shared = sd.boundary_ratio(c1, 8.0)
    below = np.nextafter(r, np.float32(0))
    assert float(r) * 8.0 == v and shared >= 2
    want_b, want_c = sd.oversize(c1, limit(r, info)), sd.oversize(c1, limit(below, info))
    assert want_c == want_b + shared and want_b > 0
    # B
    g, _ = start(monkeypatch, n_images, "wide", form, max_displacement_ratio=float(r))
    b = take_steps("", n_images, g, info, 2 if form == "sparse" else 1, "wide", restate=False)["steps"]
    g.close()
    assert np.array_equal(b[0]["coeffs"], c1) and b[0]["count"] == want_b, (b[0]["count"], want_b)
    if form == "sparse":
        inactive = ~a["active"]
        assert np.count_nonzero(c1[inactive]) > 100              # the shared values the second step starts from
        assert np.array_equal(b[1]["coeffs"], c2)
        assert b[1]["count"] == sd.oversize(c2, limit(r, info)) > 0, (b[1]["count"], sd.oversize(c2, limit(r, info)))
        assert sd.oversize(np.where(inactive[:, :, None], c2, np.float32(0)), limit(r, info)) > 0     # ... and some of it is theirs
    # C
    g, _ = start(monkeypatch, n_images, "wide", form, max_displacement_ratio=float(below))
    c = take_steps("", n_images, g, info, 1, "wide", restate=False)["steps"]
    g.close()
    assert np.array_equal(c[0]["coeffs"], c1) and c[0]["count"] == want_c, (c[0]["count"], want_c)
    # D
    g, _ = start(monkeypatch, n_images, "wide", form, max_displacement_ratio=float(below), guarantee_diffeomorphism=1)
    x = g.points()[0]
    assert g.updateDeformableTransforms(ALPHA) == -1.0
    assert step_scalars(g)[1] == want_c
    assert not coefficients(g, n_images).any()
    g.transformPoints()
    assert np.array_equal(g.points()[1], x)
    g.close()
    # E
    top = np.nextafter(np.float32(float(np.abs(c1).max()) / 8.0), np.float32(np.inf))
    assert sd.oversize(c1, limit(top, info)) == 0
    g, _ = start(monkeypatch, n_images, "wide", form, max_displacement_ratio=float(top), guarantee_diffeomorphism=1)
    assert g.updateDeformableTransforms(ALPHA) == a["steps"][0]["E"]
    assert step_scalars(g)[1] == 0 and np.array_equal(coefficients(g, n_images), c1)
    g.close()


# ---- fixed images ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_fixed", [1, 3])
def test_fixed_images(monkeypatch, n_fixed):
    """n_images = 0 in LatticeStepArgs: no mean (imageGroup.cxx:398).  The free images within 2 x bound of step(mean_over=None,
    first_image=n_fixed); the fixed images have no lattice and do not move; the count is over the free images."""
    n = 65
    g, info = start(monkeypatch, n, n_fixed_images=n_fixed)
    a = take_steps(f"wide_{n}_fixed_{n_fixed}", n, g, info, 2, "wide", first=n_fixed)
    po = sd.build(n)[0]
    for i in range(n_fixed):                                    # fixed_images_have_no_lattice: the context owns [n_fixed, n)
        with pytest.raises(_abi.FrogError):
            g.grid(i, 0)
    x, x2 = g.points()
    assert np.array_equal(x2[:po[n_fixed]], x[:po[n_fixed]])    # ... which is the zero lattice's transform
    g.close()
    c1 = a["steps"][0]["coeffs"]
    assert list(info.spacing) == [8.0] * 3 and not c1[:n_fixed].any()
    assert np.abs(c1[n_fixed:].astype(np.float64).sum(axis=0)).max() > 1e-4      # no mean was removed
    r, v, shared = sd.boundary_ratio(c1[n_fixed:], 8.0)
    for ratio in (r, np.nextafter(r, np.float32(0))):
        g, _ = start(monkeypatch, n, n_fixed_images=n_fixed, max_displacement_ratio=float(ratio))
        b = take_steps("", n, g, info, 1, "wide", first=n_fixed, restate=False)["steps"]
        g.close()
        want = sd.oversize(c1[n_fixed:], limit(ratio, info))
        assert np.array_equal(b[0]["coeffs"], c1) and b[0]["count"] == want > 0, (float(ratio), b[0]["count"], want)


# ---- contexts that own sub-ranges -------------------------------------------------------------------------------------------

RANGES = ((0, 9), (9, 19), (19, 30), (30, 51), (51, 65))        # owned: 9, 10, 11, 21, 14 -- around CP_BATCH = 10 and 2 * 10 + 1


def sharded_step(n_images, box, comm_mode=0, **opt):
    """One deformable step of the group split over RANGES, five contexts in this process on one device, driven through the
    split-phase C ABI with the collectives done here: sums in rank order, in f64, on the device."""
    import torch
    from frog_amd.distributed import HipEngine
    lib = _abi.hip_lib()
    pairs = sd.pairs(n_images)
    po, xyz, blocks = sd.build(n_images)
    options = _abi.FrogOptions.default(**{**sd.OPTIONS, **opt})
    engines = [HipEngine(pairs, options, 0, r) for r in RANGES]

    def all_reduce(tensors):
        total = torch.zeros_like(tensors[0])
        for t in tensors:
            total += t
        for t in tensors:
            t.copy_(total)
        return total

    infos = []
    for e in engines:
        e.linear_init((0.5, 0.5, 0.5))
        e.set_points2(xyz)                                      # every replica whole and identical: the frame
        e.update_stats_local()
    all_reduce([e.em for e in engines])                         # (the weights are 1 whatever the mixtures)
    for e in engines:
        e.stats_publish()
        if comm_mode:
            _abi.check(lib.frog_comm_mode(e._ctx, 1), "frog_comm_mode")
        infos.append(e.deformable_setup_bounds(0, *box))
        e.gridsum, _ = e._buffer(_abi.FROG_BUF_GRIDSUM, "<f8", 1)
    n_cp = int(np.prod(list(infos[0].dims)))
    for e in engines:
        assert e.gridsum.numel() == 3 * n_cp + (4 if comm_mode else 0)
        assert all(np.array_equal(e.matrix(i), np.eye(4)) for i in range(e.image_begin, e.image_end))
        e.phase_a(ALPHA)
    all_reduce([e.gridsum for e in engines])                    # with frog_comm_mode(ctx, 1) the energy tail is summed with the rest
    if not comm_mode:
        all_reduce([e.energy[:2] for e in engines])
    for e in engines:
        e.phase_b()
    scalars = [e.energy.cpu().numpy().copy() for e in engines]
    all_reduce([e.energy[2:3] for e in engines])
    E = [e.phase_c() for e in engines]
    coeffs = np.zeros((n_images, n_cp, 3), np.float32)
    sums = np.zeros((int(po[-1]), 4), np.float32)
    xs = []
    for e in engines:
        for i in range(e.image_begin, e.image_end):
            coeffs[i] = e.grid(i, 0)[1]
        s = np.empty_like(sums)
        _abi.check(lib.frog_get_point_sums(e._ctx, s.ctypes.data_as(_abi.c_float_p)), "frog_get_point_sums")
        sums[e.pt_begin:e.pt_end] = s[e.pt_begin:e.pt_end]
        xs.append(e.points()[0])
        e.close()
    return {"E": E, "scalars": scalars, "coeffs": coeffs, "sums": sums, "infos": infos, "xs": xs}


def test_contexts_that_own_sub_ranges(monkeypatch):
    """cp_center_kernel: batches of 10 images loaded through min(i0 + b, n_owned - 1), the GROUP's image count as the divisor,
    the count per context, the energy tail put back with two collectives per iteration."""
    n = 65
    whole = run_case(monkeypatch, n, "wide", "default")
    info, box, x = whole["info"], whole["box"], whole["x"]
    po, xyz, blocks = sd.build(n)
    lat = ld.Lattice.of(info)
    e_whole = whole["steps"][0]["E"]
    same_e = lambda e: abs(e - e_whole) <= 1e-12 * e_whole

    def same_info(i):
        return list(i.dims) == list(info.dims) and list(i.origin) == list(info.origin) and list(i.spacing) == list(info.spacing) \
            and list(i.bbox) == list(info.bbox)

    # A: the guard off
    a = sharded_step(n, box)
    assert all(same_info(i) for i in a["infos"]) and all(np.array_equal(v, x) for v in a["xs"])
    assert np.array_equal(a["sums"][:, 3], sd.links_per_point(po, blocks).astype(np.float32))
    r = ld.step(lat, po, x, a["sums"], np.zeros_like(a["coeffs"]), ALPHA, mean_over=n)
    assert np.all((r["gw"] == 0) | (r["gw"] >= 2.0 ** -140))
    act = sd.active(lat, po, x)
    arm_at = sd.layout(0, n)[0]["arms"]
    arm_nodes = sd.active(lat, np.array([0, po[1] - arm_at]), x[arm_at:po[1]])[0]
    for k, (b, e) in enumerate(RANGES):                         # a context that divided by its own count fails by far more
        ratio, at = ld.worst_ratio(r["new"][b:e], r["bound"][b:e], a["coeffs"][b:e])
        where = sd.node_class(act, int(at[1]), arm_nodes)
        print(f"context {k} owning {e - b} images: err / bound {ratio:.3f} in image {b + at[0]} at node {at[1]} ({where})")
        assert ratio <= 2.0, (k, ratio, at, where)
        note(f"step_design_shard_{k}_of_{e - b}_images", f"worst err/bound {ratio:.3f} in image {b + at[0]} at {where}")
        assert same_e(a["E"][k]), (k, a["E"][k], e_whole)
    c1 = a["coeffs"]
    assert np.abs(c1.astype(np.float64).sum(axis=0)).max() < 1e-5        # the group's mean is gone
    # the count at the boundary ratios, per context and summed
    ratio, v, shared = sd.boundary_ratio(c1, 8.0)
    below = np.nextafter(ratio, np.float32(0))
    top = np.nextafter(np.float32(float(np.abs(c1).max()) / 8.0), np.float32(np.inf))
    assert list(info.spacing) == [8.0] * 3 and float(ratio) * 8.0 == v and shared >= 2
    want = {float(q): [sd.oversize(c1[b:e], limit(q, info)) for b, e in RANGES] for q in (ratio, below, top)}
    assert sum(want[float(below)]) == sum(want[float(ratio)]) + shared and sum(want[float(ratio)]) > 0 and sum(want[float(top)]) == 0
    # (the last run in the sparse form: cp_center_kernel's own n_inactive term, over the images a context owns)
    for q, guard, mode, sparse in ((ratio, 0, 0, 0), (below, 1, 0, 0), (below, 1, 1, 0), (top, 1, 1, 0), (ratio, 0, 0, 1)):
        if sparse:
            monkeypatch.setenv("FROG_LATTICE_SPARSE", "1")
        s = sharded_step(n, box, comm_mode=mode, max_displacement_ratio=float(q), guarantee_diffeomorphism=guard)
        counts = [float(sc[2]) for sc in s["scalars"]]
        assert counts == want[float(q)], (float(q), guard, mode, counts, want[float(q)])
        assert sum(counts) == sd.oversize(c1, limit(q, info))
        for k, sc in enumerate(s["scalars"]):                   # the group's energy sums in every context: all-reduced, or put back
            assert same_e(float(np.sqrt(sc[0] / sc[1]))), (float(q), mode, k)
        if guard and sum(counts):
            assert s["E"] == [-1.0] * len(RANGES) and not s["coeffs"].any()
        else:
            assert all(same_e(e) for e in s["E"]) and np.array_equal(s["coeffs"], c1)
