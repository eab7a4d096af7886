"""What every group accumulator refuses in an add, and that a refused add leaves nothing behind: one table over Average,
CoverAverage and Labels (include/frog_chain.h).  Every case is an argument the library turns down before any launch."""
import ctypes as C

import numpy as np
import pytest

from frog_amd import _abi
from frog_amd.chain import Chain, Link
from frog_amd.volume import Average, CoverAverage, Labels

pytestmark = pytest.mark.gpu
DIMS = (5, 4, 3)                                                    # 60 voxels: one block
ORIGIN, SPACING = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
GRID = (DIMS, ORIGIN, SPACING)
N = 3


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def raw_add(name, acc, chain, src, background=0.0, out=None):
    """The library's add of accumulator `name` on views the caller built; the return code, nothing raised."""
    h, c = acc._h, chain._h if chain is not None else None
    s, o = C.byref(src), C.byref(out) if out is not None else None
    if name == "average":
        return acc._lib.frog_average_add(h, c, s, 1, background, o)
    if name == "cover":
        return acc._lib.frog_cover_add(h, c, s, None, 1, background, o)
    return acc._lib.frog_labels_add(h, c, s, background, o)


def create(name, device=0):
    return {"average": lambda: Average(GRID, N, device), "cover": lambda: CoverAverage(GRID, device),
            "labels": lambda: Labels(GRID, N, 0, device)}[name]()


def outputs(name, acc):
    """Every array finish gives; for labels the table and the fused map with its agreement."""
    if name == "labels":
        acc.finish()
        return list(acc.table()) + list(acc.fused("int32"))
    return list(acc.finish())


def good_adds(name, acc, vols, identity, k):
    """Add k of the clean sequence: image 1 goes through an identity chain and returns its resliced volume."""
    if k == 1:
        out = acc.add(vols[k], identity, resliced=True)
        assert same(out, vols[k])
    else:
        acc.add(vols[k])


@pytest.mark.parametrize("name", ["average", "cover", "labels"])
def test_refused_adds_leave_nothing_behind(name):
    rng = np.random.default_rng(47)
    shape = DIMS[::-1]
    vols = [rng.choice([0, 58, 86, 170], size=shape).astype(dt) for dt in ("uint8", "int16", "uint8")]
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
    as_float = v.astype(np.float32)

    # (chain, source, background, resliced view, what frog_last_error says)
    refused = [
        (None, off_grid, 0.0, None, "volume dimensions differ from the grid's"),
        (identity, flat, 0.0, None, "bad source geometry"),
        (None, on_grid, 0.0, out_dims, "resliced volume is not grid-sized"),
        (identity, on_grid, 0.0, out_dims, "resliced volume is not grid-sized"),
        (None, on_grid, 0.0, out_dtype, "resliced volume must have the source's type"),
        (identity, on_grid, 0.0, out_null, "resliced volume must have the source's type"),
    ]
    if name == "labels":
        refused += [
            (None, _abi.volume_view(as_float, ORIGIN, SPACING), 0.0, None, "a label volume has an integer type"),
            (None, on_grid, float("nan"), None, "background is not finite"),
            (identity, on_grid, float("inf"), None, "background is not finite"),
        ]
    if elsewhere is not None:
        refused.append((elsewhere, on_grid, 0.0, None, "chain and accumulator on different devices"))

    acc = create(name)

    def refuse_all():
        for chain, src, background, out, message in refused:
            assert raw_add(name, acc, chain, src, background, out) == _abi.FROG_E_INVALID, message
            assert message in _abi.hip_lib().frog_last_error().decode()
        assert (out_ok == 77).all()

    refuse_all()                                                    # before the first add
    good_adds(name, acc, vols, identity, 0)
    refuse_all()
    good_adds(name, acc, vols, identity, 1)
    refuse_all()
    good_adds(name, acc, vols, identity, 2)                         # the third of N: no refused call counted
    if name != "cover":
        assert raw_add(name, acc, None, on_grid) == _abi.FROG_E_INVALID
        assert "more volumes than n_images" in _abi.hip_lib().frog_last_error().decode()
    got = outputs(name, acc)

    clean = create(name)
    for k in range(N):
        good_adds(name, clean, vols, identity, k)
    want = outputs(name, clean)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert same(a, b)
    if name == "labels":
        assert list(got[0]) == [0, 58, 86, 170]
