"""Mesh files through libfrog_host.so (include/frog_host.h: frog_mesh_*) and through a stand-alone sanitizer build of the same
source (tests/mesh_driver.cpp).  Every input file is written here, byte by byte, in every readable format and variant; no device.

Cut files.  A file cut at every tenth byte is never a crash.  Where every byte of the file is needed (binary PLY, binary STL)
every cut is a refusal.  A text file, and a legacy VTK file cut between two sections, can be cut into a shorter file that is
itself complete (an OBJ cut at a line end; "12" cut to "1"): such a cut is read, and what is read must then be well formed,
indices inside the points, and no larger than the whole file's mesh."""
import os
import shutil
import struct
import subprocess
import xml.etree.ElementTree as ET

import numpy as np
import pytest

from frog_amd import _abi
from frog_amd.mesh import MeshError, read_mesh, write_mesh

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F4 = np.float32

TETRA = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F4), [[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])
MIXED = (np.array([[0.1, 1e-30, -2.5], [1e10, 3, 4], [1, 1, 0], [0, 1, 0.3333333], [-1, 0.5, 7], [2, 2, 2], [5, -0.0, 1.17549435e-38],
                   [3, 3, 3]], F4),
         [[0, 1, 2, 3], [3, 2, 5, 7, 4], [4, 6, 0]])
MESHES = {"tetra": TETRA, "mixed": MIXED}


def g(v):
    return "%.9g" % float(v)


def fan(faces):
    return [[f[0], f[j], f[j + 1]] for f in faces for j in range(1, len(f) - 1)]


def merged(xyz, triangles):
    """What an STL reader returns for these triangles: points merged by bit pattern in first-occurrence order."""
    seen, points, out = {}, [], []
    for t in triangles:
        row = []
        for i in t:
            key = xyz[i].tobytes()
            if key not in seen:
                seen[key] = len(points)
                points.append(xyz[i])
            row.append(seen[key])
        out.append(row)
    return np.array(points, F4), out


# ---- the files, written by the test ---------------------------------------------------------------------------------------------

def obj_file(xyz, faces, form):
    n = len(xyz)
    lines = ["# a comment", "mtllib none.mtl", "o thing"]
    lines += ["v %s %s %s" % tuple(g(c) for c in p) for p in xyz]
    lines += ["vt 0.5 0.25", "vn 0 0 1", "g part", "usemtl none", "s off"]
    ref = {"i": lambda i: "%d" % (i + 1), "i/t": lambda i: "%d/1" % (i + 1), "i//n": lambda i: "%d//1" % (i + 1),
           "i/t/n": lambda i: "%d/1/1" % (i + 1), "negative": lambda i: "%d" % (i - n)}[form]
    lines += ["f " + " ".join(ref(i) for i in f) for f in faces]
    return ("\n".join(lines) + "\n").encode()


def ply_header(fmt, n, m, vertex_type, count_type, index_type):
    return ("ply\nformat %s 1.0\ncomment written by the test\nelement vertex %d\nproperty %s x\nproperty %s y\nproperty %s z\n"
            "property uchar red\nelement material 1\nproperty int id\nproperty list uchar float weights\nelement face %d\n"
            "property uchar flag\nproperty list %s %s vertex_indices\nend_header\n"
            % (fmt, n, vertex_type, vertex_type, vertex_type, m, count_type, index_type)).encode()


def ply_ascii(xyz, faces, vertex_type="double"):
    body = ["%s %s %s 200" % tuple(repr(float(c)) for c in p) for p in xyz]
    body += ["7 3 0.5 0.25 1e-3"]
    body += ["1 %d %s" % (len(f), " ".join(str(i) for i in f)) for f in faces]
    return ply_header("ascii", len(xyz), len(faces), vertex_type, "uchar", "int") + ("\n".join(body) + "\n").encode()


def ply_binary(xyz, faces, vertex_type="double", count_type="ushort", index_type="uint"):
    code = {"double": "d", "float": "f", "uchar": "B", "ushort": "H", "uint": "I", "int": "i", "short": "h"}
    out = ply_header("binary_little_endian", len(xyz), len(faces), vertex_type, count_type, index_type)
    for p in xyz:
        out += struct.pack("<3" + code[vertex_type], *[float(c) for c in p]) + b"\xc8"
    out += struct.pack("<iB3f", 7, 3, 0.5, 0.25, 1e-3)
    for f in faces:
        out += struct.pack("<B" + code[count_type] + str(len(f)) + code[index_type], 1, len(f), *f)
    return out


def stl_binary(xyz, faces):
    tri = fan(faces)
    out = b"test".ljust(80, b"\0") + struct.pack("<I", len(tri))
    for t in tri:
        out += struct.pack("<3f", 0, 0, 0) + b"".join(xyz[i].tobytes() for i in t) + b"\0\0"
    return out


def stl_ascii(xyz, faces):
    lines = ["solid test mesh"]
    for t in fan(faces):
        lines += [" facet normal 0 0 0", "  outer loop"] + ["   vertex %s %s %s" % tuple(g(c) for c in xyz[i]) for i in t] + ["  endloop", " endfacet"]
    return ("\n".join(lines) + "\nendsolid test mesh\n").encode()


def vtk_file(xyz, faces, binary, point_type="float", layout="classic", strips=None):
    out = ("# vtk DataFile Version %s\na title\n%s\nDATASET POLYDATA\nPOINTS %d %s\n"
           % ("5.1" if layout == "offsets" else "3.0", "BINARY" if binary else "ASCII", len(xyz), point_type)).encode()
    if binary:
        out += xyz.astype(">f4" if point_type == "float" else ">f8").tobytes() + b"\n"
    else:
        out += ("\n".join("%s %s %s" % tuple(repr(float(c)) for c in p) for p in xyz) + "\n").encode()

    def section(name, cells):
        if layout == "classic":
            flat = [v for c in cells for v in [len(c)] + list(c)]
            head = ("%s %d %d\n" % (name, len(cells), len(flat))).encode()
            if binary:
                return head + np.array(flat, ">i4").tobytes() + b"\n"
            return head + ("\n".join("%d %s" % (len(c), " ".join(str(i) for i in c)) for c in cells) + "\n").encode()
        offsets = np.cumsum([0] + [len(c) for c in cells])
        ids = [i for c in cells for i in c]
        head = ("%s %d %d\n" % (name, len(offsets), len(ids))).encode()
        if binary:
            return (head + b"OFFSETS vtktypeint64\n" + offsets.astype(">i8").tobytes() + b"\nCONNECTIVITY vtktypeint64\n"
                    + np.array(ids, ">i8").tobytes() + b"\n")
        return (head + b"OFFSETS vtktypeint64\n" + " ".join(str(o) for o in offsets).encode() + b"\nCONNECTIVITY vtktypeint64\n"
                + " ".join(str(i) for i in ids).encode() + b"\n")

    out += section("LINES", [[0, 1]])                       # read past
    out += section("POLYGONS", faces)
    if strips:
        out += section("TRIANGLE_STRIPS", strips)
    out += ("POINT_DATA %d\nSCALARS s float 1\nLOOKUP_TABLE default\n" % len(xyz)).encode() + b"0 " * len(xyz) + b"\n"
    return out


def variants(xyz, faces):
    """name -> (extension, bytes, expected points, expected faces, every cut is a refusal)"""
    v = {}
    for form in ("i", "i/t", "i//n", "i/t/n", "negative"):
        v["obj " + form] = (".obj", obj_file(xyz, faces, form), xyz, faces, False)
    v["ply ascii"] = (".ply", ply_ascii(xyz, faces), xyz, faces, False)
    v["ply ascii float"] = (".ply", ply_ascii(xyz, faces, "float"), xyz, faces, False)
    v["ply binary"] = (".ply", ply_binary(xyz, faces), xyz, faces, True)
    v["ply binary float"] = (".ply", ply_binary(xyz, faces, "float", "uchar", "int"), xyz, faces, True)
    sp, sf = merged(xyz, fan(faces))
    v["stl binary"] = (".stl", stl_binary(xyz, faces), sp, sf, True)
    v["stl ascii"] = (".stl", stl_ascii(xyz, faces), sp, sf, False)
    v["vtk ascii"] = (".vtk", vtk_file(xyz, faces, False), xyz, faces, False)
    v["vtk ascii double"] = (".vtk", vtk_file(xyz, faces, False, "double"), xyz, faces, False)
    v["vtk binary"] = (".vtk", vtk_file(xyz, faces, True), xyz, faces, False)
    v["vtk binary double"] = (".vtk", vtk_file(xyz, faces, True, "double"), xyz, faces, False)
    v["vtk ascii offsets"] = (".vtk", vtk_file(xyz, faces, False, layout="offsets"), xyz, faces, False)
    v["vtk binary offsets"] = (".vtk", vtk_file(xyz, faces, True, layout="offsets"), xyz, faces, False)
    return v


ALL = [(m, name) for m in MESHES for name in variants(*MESHES[m])]


def as_lists(faces):
    return [[int(i) for i in f] for f in faces]


def same_mesh(got, xyz, faces):
    return got[0].dtype == F4 and got[0].tobytes() == np.asarray(xyz, F4).tobytes() and as_lists(got[1]) == as_lists(faces)


def put(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


# ---- reading --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mesh,name", ALL)
def test_read_every_format_and_variant(tmp_path, mesh, name):
    ext, data, xyz, faces, _ = variants(*MESHES[mesh])[name]
    got = read_mesh(put(tmp_path / ("in" + ext), data))
    assert same_mesh(got, xyz, faces)
    if mesh == "tetra":
        assert isinstance(got[1], np.ndarray) and got[1].shape == (4, 3) and got[1].dtype == np.uint32
    elif ext != ".stl":
        assert isinstance(got[1], list)


@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("layout", ["classic", "offsets"])
def test_vtk_triangle_strips_are_expanded(tmp_path, binary, layout):
    xyz, faces = MIXED
    data = vtk_file(xyz, faces, binary, layout=layout, strips=[[0, 1, 2, 3, 4], [5, 6, 7]])
    got = read_mesh(put(tmp_path / "strips.vtk", data))
    assert same_mesh(got, xyz, faces + [[0, 1, 2], [2, 1, 3], [2, 3, 4], [5, 6, 7]])


def test_extension_is_case_insensitive(tmp_path):
    assert same_mesh(read_mesh(put(tmp_path / "A.OBJ", obj_file(*TETRA, "i"))), *TETRA)


# ---- writing --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mesh", list(MESHES))
@pytest.mark.parametrize("ext", [".obj", ".ply", ".vtk"])
def test_written_files_read_back_exactly(tmp_path, mesh, ext):
    xyz, faces = MESHES[mesh]
    path = str(tmp_path / ("out" + ext))
    write_mesh(path, xyz, faces)
    assert same_mesh(read_mesh(path), xyz, faces)


@pytest.mark.parametrize("mesh", list(MESHES))
def test_written_stl_is_the_fan_with_normals(tmp_path, mesh):
    xyz, faces = MESHES[mesh]
    path = str(tmp_path / "out.stl")
    write_mesh(path, xyz, faces)
    assert same_mesh(read_mesh(path), *merged(xyz, fan(faces)))
    raw = open(path, "rb").read()
    n, = struct.unpack_from("<I", raw, 80)
    assert n == len(fan(faces)) and len(raw) == 84 + 50 * n and not raw.startswith(b"solid")
    if mesh == "tetra":                                     # outward unit normals of the tetrahedron's faces
        normals = np.frombuffer(raw, np.dtype([("n", "<f4", 3), ("v", "<f4", 9), ("a", "<u2")]), n, 84)["n"]
        want = np.array([[0, 0, -1], [0, -1, 0], [1, 1, 1] / np.sqrt(F4(3)), [-1, 0, 0]], F4)
        assert np.allclose(normals, want, atol=1e-6)


@pytest.mark.parametrize("mesh", list(MESHES))
def test_written_vtp_parses_as_xml(tmp_path, mesh):
    xyz, faces = MESHES[mesh]
    path = str(tmp_path / "out.vtp")
    write_mesh(path, xyz, faces)
    root = ET.parse(path).getroot()
    assert root.tag == "VTKFile" and root.get("type") == "PolyData"
    piece = root.find("PolyData/Piece")
    assert int(piece.get("NumberOfPoints")) == len(xyz) and int(piece.get("NumberOfPolys")) == len(faces)
    points = piece.find("Points/DataArray")
    assert points.get("format") == "ascii" and points.get("NumberOfComponents") == "3"
    assert np.array(points.text.split(), np.float64).astype(F4).tobytes() == xyz.tobytes()
    arrays = {a.get("Name"): [int(t) for t in a.text.split()] for a in piece.findall("Polys/DataArray")}
    assert arrays["connectivity"] == [i for f in faces for i in f]
    assert arrays["offsets"] == list(np.cumsum([len(f) for f in faces]))


def test_obj_text_keeps_every_f32(tmp_path):
    rng = np.random.default_rng(3)
    xyz = rng.integers(0, 2 ** 32, (600, 3), dtype=np.uint64).astype(np.uint32).view(F4)
    xyz = np.where(np.isfinite(xyz), xyz, F4(0.1)).astype(F4)
    xyz[:3] = [[0.1, 1e-30, 1e-45], [-0.0, 3.4028235e38, 1.17549435e-38], [1 / 3, 2 / 3, 16777217]]
    for ext in (".obj", ".vtk", ".ply"):
        path = str(tmp_path / ("bits" + ext))
        write_mesh(path, xyz, np.zeros((0, 3), np.uint32))
        assert read_mesh(path)[0].tobytes() == xyz.tobytes(), ext


# ---- refusals -------------------------------------------------------------------------------------------------------------------

def cut_files(tmp, mesh, name):
    ext, data, xyz, faces, strict = variants(*MESHES[mesh])[name]
    return [(put(tmp / ("%s_%s_%d%s" % (mesh, name.replace(" ", "_").replace("/", "-"), n, ext)), data[:n]), strict)
            for n in range(0, len(data), 10) if n < len(data)]


def well_formed(got, xyz, faces):
    p, f = got
    rows = as_lists(f)
    return len(p) <= len(xyz) + 0 and len(rows) <= len(faces) and all(0 <= i < len(p) for r in rows for i in r)


@pytest.mark.parametrize("mesh,name", ALL)
def test_cut_files_are_refused_not_crashed_on(tmp_path, mesh, name):
    ext, data, xyz, faces, strict = variants(*MESHES[mesh])[name]
    refused = 0
    for path, _ in cut_files(tmp_path, mesh, name):
        try:
            got = read_mesh(path)
        except MeshError as e:
            assert e.code == _abi.FROG_E_INVALID and ": " in str(e)
            refused += 1
            continue
        assert not strict, path
        assert well_formed(got, xyz, faces), path
    assert refused > 0


def test_index_out_of_range_is_refused(tmp_path):
    xyz, faces = TETRA
    bad = [[0, 2, 1], [0, 1, 4]]
    cases = {"a.obj": obj_file(xyz, bad, "i"), "b.obj": b"v 0 0 0\nv 1 0 0\nv 0 1 0\nf -1 -2 -4\n", "z.obj": b"v 0 0 0\nf 0 1 1\n",
             "a.ply": ply_ascii(xyz, bad), "b.ply": ply_binary(xyz, bad), "c.ply": ply_binary(xyz, [[0, 1, -1]], index_type="int"),
             "a.vtk": vtk_file(xyz, bad, False), "b.vtk": vtk_file(xyz, bad, True), "c.vtk": vtk_file(xyz, bad, True, layout="offsets")}
    for name, data in cases.items():
        with pytest.raises(MeshError) as e:
            read_mesh(put(tmp_path / name, data))
        assert e.value.code == _abi.FROG_E_INVALID, name


def corrupt_files(tmp):
    xyz, faces = TETRA
    good = ply_binary(xyz, faces, "float", "uint", "int")
    at = len(good) - (4 + 12)                                # the last face's count
    long_list = good[:at] + struct.pack("<I", 0x7FFFFFFF) + good[at + 4:]
    huge = ply_header("binary_little_endian", 2 ** 31 - 1, 1, "float", "uchar", "int") + b"\0" * 64
    vtk = vtk_file(xyz, faces, True)
    files = {"long_list.ply": long_list, "huge_count.ply": huge, "big_endian.ply": good.replace(b"binary_little_endian", b"binary_big_endian"),
             "ascii_long_list.ply": ply_ascii(xyz, faces).replace(b"1 3 1 2 3", b"1 9 1 2 3"),
             "no_points.vtk": b"# vtk DataFile Version 3.0\nt\nASCII\nDATASET POLYDATA\nPOLYGONS 1 4\n3 0 1 2\n",
             "cell_too_long.vtk": vtk.replace(np.array([3, 0, 2, 1], ">i4").tobytes(), np.array([99, 0, 2, 1], ">i4").tobytes()),
             "huge_points.vtk": b"# vtk DataFile Version 3.0\nt\nBINARY\nDATASET POLYDATA\nPOINTS 4000000000 float\n" + b"\0" * 48,
             "structured.vtk": b"# vtk DataFile Version 3.0\nt\nASCII\nDATASET STRUCTURED_POINTS\n",
             "wrong_size.stl": stl_binary(xyz, faces)[:-1] + b"\0\0", "two_vertices.stl": b"solid a\nfacet normal 0 0 0\nouter loop\nvertex 0 0 0\nvertex 1 0 0\nendloop\nendfacet\nendsolid a\n",
             "text.obj": b"v 0 zero 0\n", "empty.ply": b"", "empty.stl": b"", "empty.vtk": b""}
    return [put(tmp / name, data) for name, data in files.items()]


def test_corrupt_files_are_refused(tmp_path):
    for path in corrupt_files(tmp_path):
        with pytest.raises(MeshError) as e:
            read_mesh(path)
        assert e.value.code == _abi.FROG_E_INVALID, path


def test_unknown_extension_and_missing_file(tmp_path):
    with pytest.raises(MeshError) as e:
        read_mesh(put(tmp_path / "mesh.off", b"OFF\n"))
    assert e.value.code == _abi.FROG_E_INVALID
    with pytest.raises(MeshError) as e:
        write_mesh(str(tmp_path / "out.off"), *TETRA)
    assert e.value.code == _abi.FROG_E_INVALID and not os.path.exists(tmp_path / "out.off")
    with pytest.raises(MeshError) as e:
        read_mesh(str(tmp_path / "absent.obj"))
    assert e.value.code == _abi.FROG_E_IO
    with pytest.raises(MeshError) as e:
        write_mesh(str(tmp_path / "bad.obj"), TETRA[0], [[0, 1, 4]])
    assert e.value.code == _abi.FROG_E_INVALID
    assert same_mesh(read_mesh(put(tmp_path / "empty.obj", b"")), np.zeros((0, 3), F4), [])


# ---- the same readers in a stand-alone program under the sanitizers --------------------------------------------------------------

@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no C++ compiler")
    exe = str(tmp_path_factory.mktemp("mesh_driver") / "driver")
    base = ["g++", "-std=c++17", "-O0", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
            "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "mesh_driver.cpp"),
            os.path.join(ROOT, "frog_amd", "csrc", "host", "mesh_io.cpp"), "-o", exe]
    # the runtimes inside the program where the compiler has them as archives: the program then starts whatever else a host
    # preloads into its processes
    for extra in (["-static-libasan", "-static-libubsan"], []):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        if r.returncode == 0:
            break
    if r.returncode != 0 and ("sanitize" in r.stderr or "asan" in r.stderr or "ubsan" in r.stderr):
        pytest.skip("the compiler cannot link with -fsanitize")
    assert r.returncode == 0, r.stderr
    return exe


def test_stand_alone_driver_under_sanitizers(driver, tmp_path):
    """The stand-alone program only: the library loaded into Python is not what the sanitizers see."""
    files, expect = [], []
    for mesh, name in ALL:
        ext, data, xyz, faces, strict = variants(*MESHES[mesh])[name]
        files.append(put(tmp_path / ("good_%d%s" % (len(files), ext)), data))
        expect.append("ok %d %d %d" % (len(xyz), len(faces), sum(len(f) for f in faces)))
        for path, _ in cut_files(tmp_path, mesh, name):
            files.append(path)
            expect.append(None)
    for path in corrupt_files(tmp_path):
        files.append(path)
        expect.append("refused %d" % _abi.FROG_E_INVALID)
    out = tmp_path / "out"
    out.mkdir()
    for leaks in ("1", "0"):                                # the leak check needs ptrace, which some hosts deny their processes
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=%s:abort_on_error=0" % leaks, UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([driver, str(out)] + files, capture_output=True, text=True, timeout=120, env=env)
        if "LeakSanitizer has encountered a fatal error" not in r.stderr:
            break
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(files)
    for path, line, want in zip(files, lines, expect):
        if want is not None:
            assert line == want, path
        else:                                               # a cut file: what the library loaded into Python says of it
            try:
                p, f = read_mesh(path)
                assert line == "ok %d %d %d" % (len(p), len(f), sum(len(r) for r in f)), path
            except MeshError as e:
                assert line == "refused %d" % e.code, path
