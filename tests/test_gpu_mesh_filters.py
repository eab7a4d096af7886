"""frog_mesh_smooth, frog_isosurface_smooth, frog_isosurface_upload and frog_isosurface_cluster (include/frog_chain.h) on the
device against the NumPy restatement (tests/mesh_restate.py), byte for byte in vertices, triangles and cluster_of; then
bin/MeshSmooth, bin/MeshDecimate and bin/IsoSurface's filter flags against the Python path."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import isosurface_restate as IR
import mesh_restate as M
from frog_amd import _abi
from frog_amd.chain import Chain
from frog_amd.mesh import cluster, isosurface, read_mesh, smooth, transform_points, write_mesh
from frog_amd.volume import read_volume, write_volume
from test_gpu_chain import _write_chain, random_chain

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F4, U4 = np.float32, np.uint32


def same(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes() for g, w in zip(got, want)) and len(got) == len(want)


def smooth_same(xyz, faces, **how):
    got = smooth(xyz, faces, **how)
    return got.dtype == F4 and got.tobytes() == M.smooth(xyz, faces, **how).tobytes()


def cluster_same(xyz, tri, cell):
    return same(cluster(xyz, tri, cell), M.cluster(xyz, tri, cell))


@pytest.fixture(scope="module")
def ball():
    xyz, tri, _ = M.blocky_ball()
    return xyz, tri, M.smooth(xyz, tri)


# ---- against the restatement ----------------------------------------------------------------------------------------------------

def test_ball(ball):
    xyz, tri, want = ball
    assert smooth(xyz, tri).tobytes() == want.tobytes() and want.tobytes() != xyz.tobytes()
    assert smooth_same(xyz, tri, iterations=3, boundary=0)              # closed: no boundary, the mode changes nothing
    assert smooth_same(xyz, tri, iterations=5, lam=0.5, mu=0.5)
    piece = tri[:900]                                                   # an open piece: both boundary rules act
    for boundary in (0, 1):
        assert smooth_same(xyz, piece, iterations=3, boundary=boundary)
    assert smooth(xyz, piece, 3, boundary=0).tobytes() != smooth(xyz, piece, 3, boundary=1).tobytes()
    assert cluster_same(want, tri, 2.0) and cluster_same(xyz, tri, 0.5)


def test_open_grid_with_noise():
    xyz, tri = M.grid(6, 6, noise=0.3)
    for boundary in (0, 1):
        assert smooth_same(xyz, tri, iterations=4, boundary=boundary)
    flat, _ = M.grid(6, 6)
    assert smooth(flat, tri, 5, boundary=0).tobytes() == flat.tobytes()
    assert cluster_same(xyz, tri, 1.7)


def test_polygons_and_odd_faces():
    rng = np.random.default_rng(2)
    xyz = rng.standard_normal((12, 3)).astype(F4)
    quad_and_pentagon = [[0, 1, 2, 3], [3, 2, 4, 5, 6]]
    three_on_an_edge = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], U4)
    repeats = np.array([[0, 1, 2], [0, 1, 2], [2, 1, 0], [3, 3, 4], [5, 5, 5], [2, 1, 6]], U4)
    mixed = [[0, 1, 2, 3], [3, 2, 4, 5, 6], [1, 7, 2], [1, 2, 7], [2, 2, 8], [5], [6, 0], []]
    for faces in (quad_and_pentagon, three_on_an_edge, repeats, mixed):
        for boundary in (0, 1):
            assert smooth_same(xyz, faces, iterations=3, boundary=boundary)
    for tri in (three_on_an_edge, repeats):
        assert cluster_same(xyz, tri, 0.8)
    # vertices 9..11 have no face: they stay, in both filters
    got = smooth(xyz, mixed, 3)
    assert got[9:].tobytes() == xyz[9:].tobytes() and got[:5].tobytes() != xyz[:5].tobytes()
    assert len(cluster(xyz, repeats, 1e-3)[0]) == 12


def test_fan_with_300_neighbours():
    xyz, tri = M.fan(300)
    for boundary in (0, 1):
        assert smooth_same(xyz, tri, iterations=3, boundary=boundary)
    assert smooth_same(xyz, tri[:-1], iterations=2)                     # opened: the hub and the rim are on the boundary
    assert cluster_same(xyz, tri, 3.0)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 65537])
def test_strips(n):
    xyz, tri = M.strip(n)
    for boundary in (0, 1):
        assert smooth_same(xyz, tri, iterations=2, boundary=boundary)
    assert cluster_same(xyz, tri, 0.7)
    assert cluster_same(xyz, tri, 1e6)                                  # one cluster: one thread's sum over all n
    new, out, _ = cluster(xyz, tri, 0.05)                               # every vertex in its own cell
    assert len(new) == n and len(out) == len(tri) and same((new, out), M.cluster(xyz, tri, 0.05)[:2])


def test_empty_and_faceless():
    none, no_tri = np.zeros((0, 3), F4), np.zeros((0, 3), U4)
    assert smooth(none, no_tri).shape == (0, 3)
    assert same(cluster(none, no_tri, 1.0), M.cluster(none, no_tri, 1.0))
    xyz = np.random.default_rng(4).standard_normal((40, 3)).astype(F4)
    assert smooth(xyz, no_tri).tobytes() == xyz.tobytes() and smooth(xyz, []).tobytes() == xyz.tobytes()
    assert cluster_same(xyz, no_tri, 0.9)


def test_identity_smoothing(ball):
    xyz, tri, _ = ball
    with_zero = xyz.copy()
    with_zero[0, 0] = -0.0
    assert smooth(with_zero, tri, iterations=0).tobytes() == with_zero.tobytes()
    assert smooth(with_zero, tri, iterations=7, lam=0.0, mu=-0.0).tobytes() == with_zero.tobytes()
    assert smooth_same(with_zero, tri, iterations=1, lam=0.0, mu=0.25)  # one zero factor is still a pass
    # IEEE arithmetic carries what is not finite along: the same infinities and NaNs in the same places (a NaN's sign and payload
    # are the processor's, not the statement's), every other value to the bit
    strange = xyz.copy()
    strange[10] = [np.inf, np.nan, -np.inf]
    got, want = smooth(strange, tri, iterations=2), M.smooth(strange, tri, iterations=2)
    nan = np.isnan(want)
    assert 3 < nan.sum() < nan.size and np.array_equal(np.isnan(got), nan) and got[~nan].tobytes() == want[~nan].tobytes()


def test_cluster_keys_pass_32_bits():
    xyz, tri = M.far_apart()
    got = cluster(xyz, tri, 1.0)
    assert same(got, M.cluster(xyz, tri, 1.0)) and got[2].tolist() == [0, 1, 2, 1] and got[1].tolist() == [[0, 1, 2], [2, 1, 0]]


def test_two_runs_give_the_same_bytes(ball):
    xyz, tri, want = ball
    assert smooth(xyz, tri, 4).tobytes() == smooth(xyz, tri, 4).tobytes()
    assert same(cluster(want, tri, 2.0), cluster(want, tri, 2.0))


@pytest.mark.parametrize("stride", ["3", "4"])
def test_both_row_layouts_give_the_stated_bytes(ball, stride):
    """FROG_MESH_STRIDE is read once per process: a child smooths the ball, an open piece of it and the fan with 12-byte and with
    16-byte working rows, and prints the results' digests."""
    import hashlib
    xyz, tri, want = ball
    fan_xyz, fan_tri = M.fan(300)
    code = ("import sys, hashlib\nsys.path[:0] = [%r, %r]\nimport mesh_restate as M\nfrom frog_amd.mesh import smooth\n"
            "xyz, tri, _ = M.blocky_ball()\nfan = M.fan(300)\n"
            "for got in (smooth(xyz, tri), smooth(xyz, tri[:900], 3, boundary=0), smooth(fan[0], fan[1], 3)):\n"
            "    print(hashlib.sha256(got.tobytes()).hexdigest())\n" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, FROG_MESH_STRIDE=stride), cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    expected = [want, M.smooth(xyz, tri[:900], 3, boundary=0), M.smooth(fan_xyz, fan_tri, 3)]
    assert r.stdout.split() == [hashlib.sha256(e.tobytes()).hexdigest() for e in expected]


# ---- on an extracted surface, where it lies ---------------------------------------------------------------------------------------

def test_on_the_handle_equals_get_then_host_arrays():
    f, _ = IR.sphere((25, 23, 21), 8.2, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    labels = (f >= 0).astype(np.uint8)
    xyz, tri = isosurface(labels, label=1)
    assert len(tri) == 7656
    smoothed = smooth(xyz, tri, 6, 0.4, -0.45, 0)
    assert same(isosurface(labels, label=1, smooth=dict(iterations=6, lam=0.4, mu=-0.45, boundary=0)), (smoothed, tri))
    assert same(isosurface(labels, label=1, smooth=True), (smooth(xyz, tri), tri))
    assert same(isosurface(labels, label=1, smooth=6), (smooth(xyz, tri, 6), tri))
    assert same(isosurface(labels, label=1, cell=2.5), cluster(xyz, tri, 2.5)[:2])
    both = cluster(smooth(xyz, tri), tri, 2.0)
    assert same(isosurface(labels, label=1, smooth=True, cell=2.0), both[:2])
    # the chain comes last: apply on the clustered handle == transform_points on the clustered vertices
    chain = Chain(random_chain(np.random.default_rng(31), 2, 2.0))
    got = isosurface(labels, label=1, smooth=True, cell=2.0, chain=chain)
    assert same(got, (transform_points(chain, both[0]), both[1]))
    # a level surface that touches the grid's border: open, so the boundary rule acts on the handle too
    cut = f[:, :, :13].copy()
    xyz, tri = isosurface(cut, level=0.0)
    assert not IR.is_closed(tri)
    for boundary in (0, 1):
        assert same(isosurface(cut, level=0.0, smooth=dict(iterations=3, boundary=boundary)), (M.smooth(xyz, tri, 3, boundary=boundary), tri))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------

def test_refusals():
    lib = _abi.hip_lib()
    xyz, tri = M.octahedron(8.0)
    ptr = (np.arange(len(tri) + 1) * 3).astype(U4)
    fp, up = _abi.c_float_p, _abi.c_u32_p

    def smooth_rc(p=xyz, n=6, ptr=ptr, idx=tri, m=8, lam=0.5, mu=-0.53, boundary=1):
        p = None if p is None else p.copy()
        return lib.frog_mesh_smooth(None if p is None else p.ctypes.data_as(fp), n, None if ptr is None else ptr.ctypes.data_as(up),
                                    None if idx is None else idx.ctypes.data_as(up), m, 2, lam, mu, boundary, 0)

    assert smooth_rc() == 0
    bad = tri.copy()
    bad[5, 1] = 6
    assert smooth_rc(idx=bad) == _abi.FROG_E_INVALID and b"face index" in lib.frog_last_error()
    assert smooth_rc(p=None) == _abi.FROG_E_INVALID and smooth_rc(ptr=None) == _abi.FROG_E_INVALID and smooth_rc(idx=None) == _abi.FROG_E_INVALID
    descends = ptr.copy()
    descends[2] = 1
    assert smooth_rc(ptr=ptr + U4(1)) == _abi.FROG_E_INVALID and smooth_rc(ptr=descends) == _abi.FROG_E_INVALID
    for value in (np.nan, np.inf):
        assert smooth_rc(lam=value) == _abi.FROG_E_INVALID and smooth_rc(mu=value) == _abi.FROG_E_INVALID
    assert smooth_rc(boundary=2) == _abi.FROG_E_INVALID and smooth_rc(boundary=-1) == _abi.FROG_E_INVALID

    def upload(p, t):
        h = C.c_void_p()
        return lib.frog_isosurface_upload(p.ctypes.data_as(fp), len(p), t.ctypes.data_as(up), len(t), 0, C.byref(h)), h

    rc, h = upload(xyz, bad)
    assert rc == _abi.FROG_E_INVALID and not h.value
    assert lib.frog_isosurface_upload(None, 6, tri.ctypes.data_as(up), 8, 0, C.byref(h)) == _abi.FROG_E_INVALID
    assert lib.frog_isosurface_upload(xyz.ctypes.data_as(fp), 6, tri.ctypes.data_as(up), 8, 0, None) == _abi.FROG_E_INVALID
    rc, h = upload(xyz, tri)
    assert rc == 0
    n, m = C.c_uint32(), C.c_uint32()
    for cell in (0.0, -1.0, np.nan, np.inf, 16.0 / 2 ** 21 * 0.99):     # the last: more than 2^21 cells on an axis
        assert lib.frog_isosurface_cluster(h, cell, C.byref(n), C.byref(m), None) == _abi.FROG_E_INVALID, cell
    assert lib.frog_isosurface_cluster(None, 1.0, C.byref(n), C.byref(m), None) == _abi.FROG_E_INVALID
    assert lib.frog_isosurface_cluster(h, 1.0, None, C.byref(m), None) == _abi.FROG_E_INVALID
    assert lib.frog_isosurface_smooth(None, 1, 0.5, -0.53, 1) == _abi.FROG_E_INVALID
    assert lib.frog_isosurface_smooth(h, 1, np.nan, -0.53, 1) == _abi.FROG_E_INVALID
    assert lib.frog_isosurface_smooth(h, 1, 0.5, -0.53, 3) == _abi.FROG_E_INVALID
    # after every refusal the handle still holds its mesh; 2^21 cells on an axis are accepted
    got = np.empty((6, 3), F4), np.empty((8, 3), U4)
    assert lib.frog_isosurface_get(h, got[0].ctypes.data_as(fp), got[1].ctypes.data_as(up)) == 0 and same(got, (xyz, tri))
    assert lib.frog_isosurface_cluster(h, 16.0 / (2 ** 21 - 1), C.byref(n), C.byref(m), None) == 0 and (n.value, m.value) == (6, 8)
    lib.frog_isosurface_destroy(h)
    broken = xyz.copy()
    broken[3, 1] = np.nan
    rc, h = upload(broken, tri)
    assert rc == 0 and lib.frog_isosurface_cluster(h, 1.0, C.byref(n), C.byref(m), None) == _abi.FROG_E_INVALID
    assert b"not finite" in lib.frog_last_error()
    lib.frog_isosurface_destroy(h)
    with pytest.raises(ValueError):
        cluster(xyz, np.array([[0, 1, 2, 3]], U4), 1.0)                 # a quad


# ---- the tools ------------------------------------------------------------------------------------------------------------------

def run(exe, args, cwd):
    return subprocess.run([os.path.join(ROOT, "bin", exe)] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("ext", [".obj", ".ply"])
def test_tool_mesh_smooth_and_decimate(tmp_path, ball, ext):
    xyz, tri, _ = ball
    write_mesh(tmp_path / ("in" + ext), xyz, tri)
    xyz, tri = read_mesh(tmp_path / ("in" + ext))                       # as the tools read it (.obj holds %.9g)
    r = run("MeshSmooth", ["in" + ext, "-o", "tool" + ext], tmp_path)
    assert r.returncode == 0 and "3830 vertices" in r.stdout, r.stdout + r.stderr
    write_mesh(tmp_path / ("python" + ext), smooth(xyz, tri), tri)
    assert (tmp_path / ("tool" + ext)).read_bytes() == (tmp_path / ("python" + ext)).read_bytes()
    r = run("MeshSmooth", ["in" + ext, "-n", "3", "-l", "0.4", "-m", "-0.45", "-b", "0", "-o", "tool" + ext], tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    write_mesh(tmp_path / ("python" + ext), smooth(xyz, tri, 3, 0.4, -0.45, 0), tri)
    assert (tmp_path / ("tool" + ext)).read_bytes() == (tmp_path / ("python" + ext)).read_bytes()
    r = run("MeshDecimate", ["in" + ext, "-c", "2.0", "-o", "tool" + ext], tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    new, out, _ = cluster(xyz, tri, 2.0)
    write_mesh(tmp_path / ("python" + ext), new, out)
    assert (tmp_path / ("tool" + ext)).read_bytes() == (tmp_path / ("python" + ext)).read_bytes()
    assert "3830 vertices, 7656 triangles" in r.stdout and "%d vertices, %d triangles" % (len(new), len(out)) in r.stdout


def test_tool_polygons_and_refusals(tmp_path):
    xyz = np.random.default_rng(6).standard_normal((7, 3)).astype(F4)
    faces = [[0, 1, 2, 3], [3, 2, 4, 5, 6]]
    write_mesh(tmp_path / "poly.obj", xyz, faces)
    xyz, _ = read_mesh(tmp_path / "poly.obj")
    r = run("MeshSmooth", ["poly.obj", "-n", "2"], tmp_path)            # the default output name; the faces pass untouched
    assert r.returncode == 0, r.stdout + r.stderr
    got = read_mesh(tmp_path / "output.obj")
    assert [list(q) for q in got[1]] == faces and got[0].tobytes() == smooth(xyz, faces, 2).tobytes()
    r = run("MeshDecimate", ["poly.obj", "-c", "1.0"], tmp_path)
    assert r.returncode != 0 and "triangles only" in r.stdout
    for args in (["poly.obj", "-c", "0"], ["absent.obj", "-c", "1"], ["poly.obj", "-o", "x.obj"]):
        r = run("MeshDecimate", args, tmp_path)
        assert r.returncode != 0 and ("Error : " in r.stdout or "Usage" in r.stdout)
    r = run("MeshSmooth", ["poly.obj", "-b", "2"], tmp_path)
    assert r.returncode != 0 and "Error : " in r.stdout


@pytest.mark.parametrize("ext", [".obj", ".ply"])
def test_tool_iso_surface_filters(tmp_path, ext):
    labels = np.zeros((21, 23, 25), np.int16)
    f, _ = IR.sphere((25, 23, 21), 8.2, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    labels[f >= 0] = 2
    labels[1:3, 1:4, 1:5] = 5           # clear of the ball
    write_volume(tmp_path / "labels.nii.gz", labels, (5.0, 6.0, 7.0), (4.0, 4.0, 4.0))
    volume = read_volume(tmp_path / "labels.nii.gz")
    links = random_chain(np.random.default_rng(31), 2, 2.0)
    _write_chain(tmp_path / "t.json", links)
    how = dict(iterations=5, lam=0.45, mu=-0.5, boundary=0)
    flags = ["-s", "5", "-sl", "0.45", "-sm", "-0.5", "-sb", "0", "-c", "9.0"]
    for extra, chain in (([], None), (["-t", "t.json"], Chain(links))):
        r = run("IsoSurface", ["labels.nii.gz", "-v", "2"] + flags + extra + ["-o", "tool" + ext], tmp_path)
        assert r.returncode == 0, r.stdout + r.stderr
        xyz, tri = isosurface(volume, label=2, smooth=how, cell=9.0, chain=chain)
        write_mesh(tmp_path / ("python" + ext), xyz, tri)
        assert (tmp_path / ("tool" + ext)).read_bytes() == (tmp_path / ("python" + ext)).read_bytes()
        assert "%d vertices, %d triangles" % (len(xyz), len(tri)) in r.stdout and 0 < len(tri) < 7656
    r = run("IsoSurface", ["labels.nii.gz", "-v", "all", "-s", "20", "-c", "6.0", "-o", "organ" + ext], tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    for value in (2, 5):
        xyz, tri = isosurface(volume, label=value, smooth=True, cell=6.0)
        write_mesh(tmp_path / ("python" + ext), xyz, tri)
        assert (tmp_path / ("organ_%d%s" % (value, ext))).read_bytes() == (tmp_path / ("python" + ext)).read_bytes()
    # without the new flags: the bytes of isosurface() + write_mesh, as before
    r = run("IsoSurface", ["labels.nii.gz", "-v", "2", "-o", "plain" + ext], tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    xyz, tri = isosurface(volume, label=2)
    write_mesh(tmp_path / ("python" + ext), xyz, tri)
    assert (tmp_path / ("plain" + ext)).read_bytes() == (tmp_path / ("python" + ext)).read_bytes() and len(tri) == 7656
    r = run("IsoSurface", ["labels.nii.gz", "-v", "2", "-c", "-1"], tmp_path)
    assert r.returncode != 0 and "Error : " in r.stdout
