"""What every group accumulator refuses, and that a refused call leaves nothing behind: one table over Average, CoverAverage,
Labels, Staple, WeightedLabels, JointLabels, RankImages and GroupGLM (include/frog_chain.h).  Most cases are arguments the
library turns down before any launch; a volume with more labels than the table holds is turned down after its collect, and
its inserts are taken back.  The text of frog_last_error is part of what is checked: where a row states the whole message, with
the entry point's name in front, the two are compared for equality."""
import ctypes as C

import numpy as np
import pytest

from frog_amd import _abi
from frog_amd.chain import Chain, Link
from frog_amd.volume import Average, CoverAverage, GroupGLM, JointLabels, Labels, RankImages, Staple, WeightedLabels

pytestmark = pytest.mark.gpu
DIMS = (5, 4, 3)                                                    # 60 voxels: one block
ORIGIN, SPACING = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
GRID = (DIMS, ORIGIN, SPACING)
N = 3
MAX_LABELS = 4                                                      # the clean volumes hold exactly four values
LABELLED = ("labels", "staple", "wlabels", "jlabels")               # accumulators with a label table
ATLASES = ("wlabels", "jlabels")                                    # an add takes an image and its label map
WINDOWED = ("rank", "glm")                                          # an add returns no resliced volume


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()       # bit for bit, NaNs included


def last_error():
    return _abi.hip_lib().frog_last_error().decode()


def raw_add(name, acc, chain, src, background=0.0, out=None, labels=None, label_background=0.0, labels_out=None):
    """The library's add of accumulator `name` on views the caller built; the return code, nothing raised."""
    h, c = acc._h, chain._h if chain is not None else None
    s, o = C.byref(src), C.byref(out) if out is not None else None
    if name == "average":
        return acc._lib.frog_average_add(h, c, s, 1, background, o)
    if name == "cover":
        return acc._lib.frog_cover_add(h, c, s, None, 1, background, o)
    if name in WINDOWED:
        return getattr(acc._lib, f"frog_{name}_add")(h, c, s, None, 1, background)
    if name in ATLASES:
        lo = C.byref(labels_out) if labels_out is not None else None
        return getattr(acc._lib, f"frog_{name}_add")(h, c, s, C.byref(labels), 1, background, label_background, o, lo)
    return getattr(acc._lib, f"frog_{name}_add")(h, c, s, background, o)


def raw_get(name, acc, what, value=0, view=None):
    """The library's getter `what` (values, fused, probability) of label accumulator `name`; the return code."""
    lib, h = acc._lib, acc._h
    p = np.empty(DIMS[::-1], np.float32)
    fp = p.ctypes.data_as(_abi.c_float_p)
    if what == "probability":
        return getattr(lib, f"frog_{name}_probability")(h, value, fp)
    if what == "fused":
        fused = getattr(lib, f"frog_{name}_fused")
        return fused(h, 0, C.byref(view), fp) if name in ATLASES else fused(h, C.byref(view), fp)
    values, counts = (C.c_int64 * 16)(), (C.c_uint64 * 16)()
    if name == "labels":                                            # its values come with the table
        return lib.frog_labels_table(h, values, counts, counts)
    return getattr(lib, f"frog_{name}_values")(h, values)


def create(name, target, device=0):
    if name in ATLASES:
        acc = WeightedLabels(GRID, N, MAX_LABELS, 1, device=device) if name == "wlabels" else JointLabels(GRID, N, MAX_LABELS, 1, device=device)
        acc.target(target)
        return acc
    return {"average": lambda: Average(GRID, N, device), "cover": lambda: CoverAverage(GRID, device),
            "labels": lambda: Labels(GRID, N, MAX_LABELS, device), "staple": lambda: Staple(GRID, N, MAX_LABELS, device),
            "rank": lambda: RankImages(GRID, N, None, device), "glm": lambda: GroupGLM(GRID, np.ones((N, 1)), None, device)}[name]()


def finish(name, acc):
    """Everything up to the point at which every output may be asked for."""
    if name in LABELLED:
        acc.finish()
    if name == "staple":
        acc.solve()


def outputs(name, acc):
    """Every array the finished accumulator gives."""
    if name == "labels":
        values = acc.table()[0]
        return list(acc.table()) + list(acc.fused("int32")) + [acc.probability(v) for v in values]
    if name in LABELLED:
        values = acc.values()
        extra = list(acc.performance()) if name == "staple" else []
        return [values] + list(acc.fused("int32")) + [acc.probability(v) for v in values] + extra
    if name == "rank":
        return list(acc.finish(quantiles=(0.25, 0.5)))
    if name == "glm":
        return list(acc.finish([[1.0]])) + [acc.plane(k) for k in range(N)]
    return list(acc.finish())


def good_adds(name, acc, vols, identity, k):
    """Add k of the clean sequence: image 1 goes through an identity chain and, where the add has one, returns its resliced
    volume.  An atlas is volume k as the image and as its own label map."""
    if name in WINDOWED:
        acc.add(vols[k], identity if k == 1 else None)
    elif name in ATLASES:
        if k == 1:
            image, labels = acc.add(vols[k], vols[k], identity, resliced=True)
            assert same(image, vols[k]) and same(labels, vols[k])
        else:
            acc.add(vols[k], vols[k])
    elif k == 1:
        out = acc.add(vols[k], identity, resliced=True)
        assert same(out, vols[k])
    else:
        acc.add(vols[k])


@pytest.mark.parametrize("name", ["average", "cover", "labels", "staple", "wlabels", "jlabels", "rank", "glm"])
def test_refused_adds_leave_nothing_behind(name):
    rng = np.random.default_rng(47)
    shape = DIMS[::-1]
    vols = [rng.choice([0, 58, 86, 170], size=shape).astype(dt) for dt in ("uint8", "int16", "uint8")]
    target = rng.normal(100.0, 30.0, size=shape).astype(np.float32)
    identity = Chain([Link.linear(np.eye(4))])
    n_devices = _abi.hip_lib().frog_device_count()
    elsewhere = Chain([Link.linear(np.eye(4))], device=1) if n_devices > 1 else None

    v = vols[1]
    on_grid = _abi.volume_view(v, ORIGIN, SPACING)
    off_grid = _abi.volume_view(np.zeros((3, 4, 6), v.dtype), ORIGIN, SPACING)
    flat = _abi.volume_view(v, ORIGIN, (1.0, 0.0, 1.0))
    out_ok = np.full(shape, 77, v.dtype)
    out_dims = _abi.volume_view(np.zeros((3, 4, 6), v.dtype), ORIGIN, SPACING)
    out_dtype = _abi.volume_view(np.zeros(shape, np.int32), ORIGIN, SPACING)
    out_null = _abi.volume_view(out_ok, ORIGIN, SPACING)
    out_null.data = None
    float_voxels = v.astype(np.float32)                             # a view keeps no reference to its array
    as_float = _abi.volume_view(float_voxels, ORIGIN, SPACING)
    crowded_voxels = rng.permutation(np.resize(np.array([0, 58, 86, 170, 201], v.dtype), v.size)).reshape(shape)
    crowded = _abi.volume_view(crowded_voxels, ORIGIN, SPACING)     # one value more than the table holds

    def rows(chain, view, background, out, message):
        """One refused add as raw_add's arguments; for an atlas two, the image and then the label map being at fault."""
        if name in ATLASES:
            return [(dict(chain=chain, src=view, labels=on_grid, background=background, out=out), message),
                    (dict(chain=chain, src=on_grid, labels=view, label_background=background, labels_out=out), message)]
        if name in WINDOWED and out is not None:
            return []
        return [(dict(chain=chain, src=view, background=background, out=out), message)]

    refused = (rows(None, off_grid, 0.0, None, "volume dimensions differ from the grid's")
               + rows(identity, flat, 0.0, None, "bad source geometry")
               + rows(None, on_grid, 0.0, out_dims, "resliced volume is not grid-sized")
               + rows(identity, on_grid, 0.0, out_dims, "resliced volume is not grid-sized")
               + rows(None, on_grid, 0.0, out_dtype, "resliced volume must have the source's type")
               + rows(identity, on_grid, 0.0, out_null, "resliced volume must have the source's type"))
    if name in LABELLED:
        overflow = f"frog_{name}_add: more than max_labels = {MAX_LABELS} distinct labels"
        refused += (rows(None, on_grid, float("nan"), None, "background is not finite")
                    + rows(identity, on_grid, float("inf"), None, "background is not finite")
                    + rows(None, as_float, 0.0, None, "a label volume has an integer type")[-1:]       # of an atlas: its label map
                    + rows(None, crowded, 0.0, None, overflow)[-1:]
                    + rows(identity, crowded, 0.0, None, overflow)[-1:])
    if elsewhere is not None:
        refused += rows(elsewhere, on_grid, 0.0, None, "chain and accumulator on different devices")

    acc = create(name, target)

    def expect(code, message):
        assert code == _abi.FROG_E_INVALID, message
        if message.startswith("frog_"):
            assert last_error() == message
        else:
            assert message in last_error()

    def refuse_all():
        for arguments, message in refused:
            expect(raw_add(name, acc, **arguments), message)
        if name in LABELLED:                                        # no output before its time
            ready = "frog_staple_solve" if name == "staple" else f"frog_{name}_finish"
            for what in ("fused", "probability"):
                expect(raw_get(name, acc, what, 58, on_grid), f"frog_{name}_{what}: before {ready}")
            what = "table" if name == "labels" else "values"
            expect(raw_get(name, acc, "values"), f"frog_{name}_{what}: before frog_{name}_finish")
        assert (out_ok == 77).all()

    refuse_all()                                                    # before the first add
    good_adds(name, acc, vols, identity, 0)
    refuse_all()
    good_adds(name, acc, vols, identity, 1)
    refuse_all()
    good_adds(name, acc, vols, identity, 2)                         # the third of N: no refused call counted
    if name != "cover":
        full = "atlases than n_images" if name in ATLASES else "volumes than the accumulator was created for" if name in WINDOWED else "volumes than n_images"
        arguments = dict(chain=None, src=on_grid, labels=on_grid) if name in ATLASES else dict(chain=None, src=on_grid)
        expect(raw_add(name, acc, **arguments), "more " + full)
    finish(name, acc)
    if name in LABELLED:
        # frog_jlabels_fused and frog_jlabels_probability make their own first checks and hand over to frog_wlabels', whose
        # name is in front of everything after them
        body = "wlabels" if name == "jlabels" else name
        missing = "no such label" if name == "staple" else "no such label in the table"
        expect(raw_get(name, acc, "probability", 59), f"frog_{body}_probability: {missing}")
        expect(raw_get(name, acc, "fused", view=as_float), f"frog_{body}_fused: the fused map has an integer type")
        expect(raw_get(name, acc, "fused", view=out_dims), f"frog_{body}_fused: the fused map is not grid-sized")
    got = outputs(name, acc)

    clean = create(name, target)
    for k in range(N):
        good_adds(name, clean, vols, identity, k)
    finish(name, clean)
    want = outputs(name, clean)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert same(a, b)
    if name in LABELLED:
        assert list(got[0]) == [0, 58, 86, 170]


@pytest.mark.parametrize("name", WINDOWED)
@pytest.mark.parametrize("first, planes", [(DIMS[2], 1), (0, 0), (1, DIMS[2]), (0, DIMS[2] + 1)])
def test_windowed_create_refuses_a_window_outside_the_grid(name, first, planes):
    lib = _abi.hip_lib()
    grid = _abi.volume_view(None, ORIGIN, SPACING, DIMS)
    h = C.c_void_p()
    if name == "rank":
        code = lib.frog_rank_create(C.byref(grid), first, planes, N, 0, C.byref(h))
    else:
        design = np.ones((N, 1))
        code = lib.frog_glm_create(C.byref(grid), first, planes, N, 1, design.ctypes.data_as(_abi.c_double_p), 0, C.byref(h))
    assert code == _abi.FROG_E_INVALID and not h
    assert last_error() == f"frog_{name}_create: the window lies outside the grid or is empty"
