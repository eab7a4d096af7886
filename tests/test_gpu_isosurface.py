"""frog_isosurface_* and frog_chain_apply_f32 (include/frog_chain.h) on the device against the NumPy restatement
(tests/isosurface_restate.py), byte for byte in counts, vertices and triangles; then bin/IsoSurface and bin/MeshTransform
against the Python path."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import isosurface_restate as R
from frog_amd import _abi
from frog_amd.chain import Chain, Link, invert
from frog_amd.mesh import isosurface, read_mesh, transform_points, write_mesh
from frog_amd.volume import read_volume, write_volume
from test_gpu_chain import _write_chain, random_chain

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F4 = np.float32


def same(got, want):
    return (got[0].dtype == F4 and got[1].dtype == np.uint32 and got[0].shape == want[0].shape and got[1].shape == want[1].shape
            and got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes())


def both(volume, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), **how):
    return isosurface((volume, origin, spacing), **how), R.isosurface(volume, origin, spacing, **how)


def raw_create(volume, origin, spacing, mode, level, value):
    """The C ABI by hand: (status, n_vertices, n_triangles, xyz, triangles)."""
    lib = _abi.hip_lib()
    v = _abi.volume_view(np.ascontiguousarray(volume), origin, spacing)
    h, n, m = C.c_void_p(), C.c_uint32(7), C.c_uint32(7)
    rc = lib.frog_isosurface_create(C.byref(v), mode, level, value, 0, C.byref(h), C.byref(n), C.byref(m))
    if rc:
        return rc, None, None, None, None
    xyz, tri = np.empty((n.value, 3), F4), np.empty((m.value, 3), np.uint32)
    assert lib.frog_isosurface_get(h, xyz.ctypes.data_as(_abi.c_float_p), tri.ctypes.data_as(_abi.c_u32_p)) == 0
    lib.frog_isosurface_destroy(h)
    return rc, n.value, m.value, xyz, tri


# ---- against the restatement ----------------------------------------------------------------------------------------------------

def test_every_cell_configuration():
    for config in range(256):
        got, want = both(R.cell_configuration(config), level=0.5)
        assert same(got, want), config
        assert (len(got[1]) == 0) == (config == 0)


@pytest.mark.parametrize("case", range(len(R.SPHERES)))
def test_spheres(case):
    dims, radius, spacing, origin = R.SPHERES[case]
    f, _ = R.sphere(dims, radius, spacing, origin)
    got, want = both(f, origin, spacing, level=0.0)
    assert same(got, want) and len(want[1]) > 500
    assert R.is_closed(got[1]) and R.euler_characteristic(*got) == 2
    rc, n, m, xyz, tri = raw_create(f, origin, spacing, _abi.FROG_ISO_LEVEL, 0.0, 0)
    assert rc == 0 and (n, m) == (len(want[0]), len(want[1])) and same((xyz, tri), want)


def test_ties():
    got, want = both(R.ties_block(), level=1.0)
    assert same(got, want) and R.is_closed(got[1]) and R.signed_volume(*got) == 8.0


@pytest.mark.parametrize("dims", [(1, 1, 1), (2, 2, 2), (1, 5, 5), (5, 1, 5), (2, 3, 65), (67, 3, 2), (3, 130, 2), (259, 2, 2), (33, 17, 9)])
def test_grids_across_block_edges(dims):
    rng = np.random.default_rng(sum(dims))
    f = rng.normal(size=dims[::-1]).astype(F4)
    got, want = both(f, (-1.0, 2.0, 0.5), (0.3, 1.7, 1.1), level=0.1)
    assert same(got, want)
    assert (len(want[1]) > 0) == (min(dims) >= 2)


@pytest.mark.parametrize("dtype", _abi.FROG_V_DTYPES)
def test_every_dtype_in_level_mode(dtype):
    rng = np.random.default_rng(11)
    base = rng.normal(size=(7, 9, 11)) * 40
    if dtype.startswith("uint"):
        base = base + 100
    f = np.clip(base, np.iinfo(dtype).min, np.iinfo(dtype).max).astype(dtype) if "int" in dtype else base.astype(dtype)
    level = 110.5 if dtype.startswith("uint") else 7.0         # 7.0: integer volumes hold voxels equal to the level
    got, want = both(f, (3.0, -2.0, 1.0), (1.25, 0.75, 2.0), level=level)
    assert same(got, want) and len(want[1]) > 100
    if "int" in dtype and not dtype.startswith("uint"):
        assert (f == 7).any()


@pytest.mark.parametrize("dtype", _abi.FROG_V_DTYPES[:6])
def test_every_integer_dtype_in_label_mode(dtype):
    rng = np.random.default_rng(13)
    info = np.iinfo(dtype)
    values = [0, 1, int(info.max), int(info.min) if info.min < 0 else 2]
    if dtype == "int32":
        values += [-5, -2 ** 31]
    if dtype == "uint32":
        values += [2 ** 31 + 5, 2 ** 32 - 1]
    labels = np.array(values, np.int64)[rng.integers(0, len(values), (6, 7, 8))].astype(dtype)
    for value in values:
        got, want = both(labels, (0.0, 1.0, 2.0), (1.0, 0.5, 2.0), label=value)
        assert same(got, want) and len(want[1]) > 0, value
        assert same(want, R.isosurface((labels.astype(np.int64) == value).astype(np.uint8), (0.0, 1.0, 2.0), (1.0, 0.5, 2.0), level=0.5))
    got, want = both(labels, label=3)                           # a value nothing carries
    assert same(got, want) and len(got[0]) == 0
    if dtype == "uint32":                                       # a value outside the type is carried by nothing
        assert len(isosurface(labels, label=-1)[0]) == 0 and len(isosurface(labels, label=2 ** 32)[0]) == 0


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_special_values(dtype):
    tiny = np.finfo(dtype).tiny
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, tiny / 4, -tiny / 4, 1.0, -1.0, np.finfo(dtype).max, -np.finfo(dtype).max], dtype)
    rng = np.random.default_rng(17)
    f = special[rng.integers(0, len(special), (8, 9, 10))]
    for level in (-0.0, 0.0, float(tiny / 4), 1.0, float("inf"), float("-inf")):
        got, want = both(f, (0.5, 0.5, 0.5), (1.0, 2.0, 3.0), level=level)
        assert same(got, want), level
    assert len(R.isosurface(f, level=-0.0)[1]) > 100


def test_surface_touching_the_border_is_open_and_equal():
    z, y, x = np.meshgrid(np.arange(10), np.arange(12), np.arange(14), indexing="ij")
    f = (6.5 - np.sqrt((x - 2.0) ** 2 + (y - 6.0) ** 2 + (z - 9.0) ** 2)).astype(F4)
    got, want = both(f, level=0.0)
    assert same(got, want) and len(want[1]) > 100 and not R.is_closed(want[1])


def test_two_runs_give_the_same_bytes():
    dims, radius, spacing, origin = R.SPHERES[2]
    f, _ = R.sphere(dims, radius, spacing, origin)
    assert same(isosurface((f, origin, spacing), level=0.0), isosurface((f, origin, spacing), level=0.0))


# ---- points through a chain in f32 ----------------------------------------------------------------------------------------------

def mixed_chain():
    """A linear link, a B-spline link, an inverse B-spline link and a field link."""
    rng = np.random.default_rng(23)
    linear, lattice = random_chain(rng, 1, 2.0)
    other = random_chain(rng, 1, 1.0)[1]
    dims = (9, 8, 7)
    field = Link.field(dims, (-10.0, -10.0, -10.0), (15.0, 17.0, 20.0), rng.normal(size=(dims[0] * dims[1] * dims[2], 3)).astype(F4))
    return [linear, lattice] + invert([other]) + [field]


def test_apply_f32_is_the_f64_path_cast_once():
    rng = np.random.default_rng(29)
    chain = Chain(mixed_chain())
    x = rng.uniform(-30, 140, (3001, 3)).astype(F4)
    x[5] = [np.nan, 10.0, 20.0]
    x[6] = [0.0, -0.0, 50.0]
    got = transform_points(chain, x)
    want = chain.apply(x.astype(np.float64)).astype(F4)
    finite = np.isfinite(want).all(axis=1)
    assert got.dtype == F4 and got[finite].tobytes() == want[finite].tobytes() and finite.sum() >= 3000
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[5, 0])
    assert np.abs(got - x)[finite].max() > 1.0                  # the chain moves points
    assert len(transform_points(chain, np.zeros((0, 3), F4))) == 0


def test_isosurface_apply_is_get_then_apply_f32():
    dims, radius, spacing, origin = (25, 23, 21), 36.0, (4.0, 4.0, 4.0), (5.0, 6.0, 7.0)
    f, _ = R.sphere(dims, radius, spacing, origin)
    chain = Chain(mixed_chain())
    plain = isosurface((f, origin, spacing), level=0.0)
    moved = isosurface((f, origin, spacing), level=0.0, chain=chain)
    assert moved[1].tobytes() == plain[1].tobytes()
    assert moved[0].tobytes() == transform_points(chain, plain[0]).tobytes()
    assert np.abs(moved[0] - plain[0]).max() > 0.5


# ---- refusals -------------------------------------------------------------------------------------------------------------------

def test_invalid_arguments():
    lib = _abi.hip_lib()
    f = np.zeros((3, 3, 3), F4); f[1, 1, 1] = 1
    v = _abi.volume_view(f, (0, 0, 0), (1, 1, 1))
    h, n, m = C.c_void_p(), C.c_uint32(), C.c_uint32()

    def create(vol=v, mode=0, level=0.5, value=0, out=C.byref(h), pn=C.byref(n), pm=C.byref(m)):
        return lib.frog_isosurface_create(None if vol is None else C.byref(vol), mode, level, value, 0, out, pn, pm)

    assert create(vol=None) == _abi.FROG_E_INVALID
    assert create(out=None) == _abi.FROG_E_INVALID
    assert create(pn=None) == _abi.FROG_E_INVALID and create(pm=None) == _abi.FROG_E_INVALID
    nodata = _abi.volume_view(f, (0, 0, 0), (1, 1, 1)); nodata.data = None
    assert create(vol=nodata) == _abi.FROG_E_INVALID
    assert create(mode=2) == _abi.FROG_E_INVALID and create(mode=-1) == _abi.FROG_E_INVALID
    for dtype in (8, -1):
        bad = _abi.volume_view(f, (0, 0, 0), (1, 1, 1)); bad.dtype = dtype
        assert create(vol=bad) == _abi.FROG_E_INVALID
    assert create(mode=_abi.FROG_ISO_LABEL) == _abi.FROG_E_INVALID                     # a float volume in label mode
    f64 = _abi.volume_view(f.astype(np.float64), (0, 0, 0), (1, 1, 1))
    assert create(vol=f64, mode=_abi.FROG_ISO_LABEL) == _abi.FROG_E_INVALID
    assert create(level=float("nan")) == _abi.FROG_E_INVALID
    for dims in ((2048, 2048, 513), (65536, 65536, 2), (2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1)):   # refused before a voxel is read
        big = _abi.volume_view(f, (0, 0, 0), (1, 1, 1)); big.dims[:] = dims
        assert create(vol=big) == _abi.FROG_E_INVALID
    assert h.value is None
    assert create() == 0 and n.value == 14 and m.value == 24    # one inside node: 14 edges cross, 24 tetrahedra hold it
    chain = Chain([Link.linear(np.eye(4))])
    assert lib.frog_isosurface_apply(None, chain._h) == _abi.FROG_E_INVALID
    assert lib.frog_isosurface_apply(h, None) == _abi.FROG_E_INVALID
    assert lib.frog_isosurface_get(None, None, None) == _abi.FROG_E_INVALID
    assert lib.frog_isosurface_get(h, None, None) == _abi.FROG_E_INVALID
    lib.frog_isosurface_destroy(h)
    lib.frog_isosurface_destroy(None)
    assert lib.frog_chain_apply_f32(None, f.ctypes.data_as(_abi.c_float_p), f.ctypes.data_as(_abi.c_float_p), 1) == _abi.FROG_E_INVALID
    assert lib.frog_chain_apply_f32(chain._h, None, f.ctypes.data_as(_abi.c_float_p), 1) == _abi.FROG_E_INVALID
    with pytest.raises(ValueError):
        isosurface(f)
    with pytest.raises(ValueError):
        isosurface(f, level=0.5, label=1)


def test_result_limit_is_found_from_the_totals():
    """The refusal of 2^31 vertices or triangles, reached on a small grid through the library's test hook (read once per
    process, hence the child): a surface below the limit passes, one at it is refused."""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import numpy as np, isosurface_restate as R\n"
            "from frog_amd import _abi\nfrom frog_amd.mesh import isosurface\n"
            "f = np.zeros((3, 3, 3), np.float32); f[1, 1, 1] = 1\n"
            "print(len(isosurface(f, level=0.5)[1]))\n"
            "f = np.zeros((3, 3, 4), np.float32); f[1, 1, 1:3] = 1\n"
            "try:\n    isosurface(f, level=0.5)\n    print('passed')\n"
            "except _abi.FrogError as e:\n    print(e.code, 'a surface holds fewer than 25' in str(e))\n") % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, FROG_ISO_RESULT_MAX="25"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split("\n")[:2] == ["24", "%d True" % _abi.FROG_E_INVALID]


# ---- the tools ------------------------------------------------------------------------------------------------------------------

def run(exe, args, cwd):
    return subprocess.run([os.path.join(ROOT, "bin", exe)] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=300)


def sphere_file(tmp_path):
    """A sphere inside the test chains' lattices, as the tools read it back from its file."""
    f, _ = R.sphere((25, 23, 21), 36.0, (4.0, 4.0, 4.0), (5.0, 6.0, 7.0))
    write_volume(tmp_path / "sphere.nii.gz", f, (5.0, 6.0, 7.0), (4.0, 4.0, 4.0))
    return read_volume(tmp_path / "sphere.nii.gz")


@pytest.mark.parametrize("ext", [".obj", ".ply"])
def test_tool_iso_surface_equals_the_python_path(tmp_path, ext):
    volume = sphere_file(tmp_path)
    links = random_chain(np.random.default_rng(31), 2, 2.0)
    _write_chain(tmp_path / "t.json", links)
    for extra, chain in (([], None), (["-t", "t.json"], Chain(links)), (["-ti", "t.json"], Chain(invert(links)))):
        r = run("IsoSurface", ["sphere.nii.gz", "-l", "0"] + extra + ["-o", "tool" + ext], tmp_path)
        assert r.returncode == 0, r.stdout + r.stderr
        xyz, tri = isosurface(volume, level=0.0, chain=chain)
        write_mesh(tmp_path / ("python" + ext), xyz, tri)
        assert (tmp_path / ("tool" + ext)).read_bytes() == (tmp_path / ("python" + ext)).read_bytes()
        assert "%d vertices, %d triangles" % (len(xyz), len(tri)) in r.stdout and len(tri) > 1000


def test_tool_iso_surface_all_values(tmp_path):
    rng = np.random.default_rng(37)
    labels = np.zeros((12, 14, 16), np.int16)
    labels[2:6, 2:7, 3:9] = 1
    labels[6:10, 4:12, 5:13] = 2
    labels[3:5, 9:12, 2:6] = -7
    write_volume(tmp_path / "labels.nii.gz", labels, (1.0, 2.0, 3.0), (0.5, 1.5, 2.0))
    volume = read_volume(tmp_path / "labels.nii.gz")
    r = run("IsoSurface", ["labels.nii.gz", "-v", "all", "-o", "organ.ply"], tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(p.name for p in tmp_path.glob("organ*")) == ["organ_-7.ply", "organ_1.ply", "organ_2.ply"]
    lines = [l for l in r.stdout.split("\n") if "vertices" in l]
    assert [l.split(" : ")[0] for l in lines] == ["organ_-7.ply", "organ_1.ply", "organ_2.ply"]      # ascending
    for value in (-7, 1, 2):
        xyz, tri = isosurface(volume, label=value)
        got = read_mesh(tmp_path / ("organ_%d.ply" % value))
        assert same((got[0], got[1]), (xyz, tri)) and R.is_closed(tri) and len(tri) > 0
    r = run("IsoSurface", ["labels.nii.gz", "-v", "2", "-o", "two.obj"], tmp_path)
    assert r.returncode == 0 and same(read_mesh(tmp_path / "two.obj"), isosurface(volume, label=2))
    r = run("IsoSurface", ["labels.nii.gz", "-l", "1", "-v", "2"], tmp_path)
    assert r.returncode != 0 and "Error" in r.stdout
    write_volume(tmp_path / "float.nii.gz", labels.astype(F4))
    r = run("IsoSurface", ["float.nii.gz", "-v", "1"], tmp_path)
    assert r.returncode != 0 and "integer type" in r.stdout


def test_tool_mesh_transform(tmp_path):
    f, _ = R.sphere((25, 23, 21), 36.0, (4.0, 4.0, 4.0), (5.0, 6.0, 7.0))
    xyz, tri = R.isosurface(f, (5.0, 6.0, 7.0), (4.0, 4.0, 4.0), level=0.0)
    assert R.is_closed(tri)
    write_mesh(tmp_path / "in.ply", xyz, tri)
    rng = np.random.default_rng(41)
    a, b = random_chain(rng, 2, 2.0), random_chain(rng, 1, 1.0)
    _write_chain(tmp_path / "a.json", a)
    _write_chain(tmp_path / "b.json", b)
    # of several -t / -ti the one given last is applied first
    r = run("MeshTransform", ["in.ply", "-t", "a.json", "-ti", "b.json", "-o", "out.ply"], tmp_path)
    assert r.returncode == 0 and "Transform computed in " in r.stdout, r.stdout + r.stderr
    got = read_mesh(tmp_path / "out.ply")
    want = transform_points(Chain(invert(b) + a), xyz)
    assert got[0].tobytes() == want.tobytes() and got[1].tobytes() == tri.tobytes() and R.is_closed(got[1])
    other = transform_points(Chain(a + invert(b)), xyz)
    assert np.abs(other - want).max() > 1e-3                    # the order matters on this pair
    r = run("MeshTransform", ["in.ply", "-ti", "b.json", "-t", "a.json", "-o", "swapped.ply"], tmp_path)
    assert r.returncode == 0 and read_mesh(tmp_path / "swapped.ply")[0].tobytes() == other.tobytes()
    # the default output name, and a polygon mesh whose faces pass untouched
    quads = [[0, 1, 2, 3], [3, 2, 1, 0, 4]]
    write_mesh(tmp_path / "poly.obj", xyz[:5], quads)
    r = run("MeshTransform", ["poly.obj", "-t", "a.json"], tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    got = read_mesh(tmp_path / "output.obj")
    assert [list(q) for q in got[1]] == quads and got[0].tobytes() == transform_points(Chain(a), xyz[:5]).tobytes()
    # a transform and its inverse: a linear-only chain returns the points to the last f32 digits
    M = np.array([[0.9, 0.1, -0.2, 3.0], [0.05, 1.1, 0.1, -2.0], [-0.1, 0.2, 1.05, 7.0], [0, 0, 0, 1.0]])
    _write_chain(tmp_path / "m.json", [Link.linear(M)])
    r = run("MeshTransform", ["in.ply", "-t", "m.json", "-ti", "m.json", "-o", "back.ply"], tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    back = read_mesh(tmp_path / "back.ply")
    assert back[1].tobytes() == tri.tobytes()
    magnitude = np.abs(xyz).max(axis=1, keepdims=True)
    assert (np.abs(back[0].astype(np.float64) - xyz) <= 2 * 2.0 ** -23 * magnitude).all()
    r = run("MeshTransform", ["absent.ply", "-t", "a.json"], tmp_path)
    assert r.returncode != 0 and "Error : " in r.stdout
