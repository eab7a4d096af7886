"""Displacement fields as chain links: the transform-file entry {"type": "frogDisplacementField", "file": ...}, the refusal to
invert a field link, and the argument checks of bin/TransformField and frog_chain_sample that need no device."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from frog_amd import _abi
from frog_amd.chain import BSPLINE, BSPLINE_INVERSE, FIELD, LINEAR, Link, invert, read_transform
from test_chain import smooth_chain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "TransformField")


def write_nifti(path, dims, origin, spacing, values):
    v = np.ascontiguousarray(values, np.float32)
    d = (C.c_uint32 * 3)(*dims); s = (C.c_double * 3)(*spacing); o = (C.c_double * 3)(*origin)
    nc = v.size // (dims[0] * dims[1] * dims[2])
    assert _abi.host_lib().frog_nifti_write(str(path).encode(), d, s, o, nc, v.ctypes.data_as(_abi.c_float_p)) == 0


def test_field_entry_is_read_by_both_readers(tmp_path):
    lib = _abi.host_lib()
    rng = np.random.default_rng(11)
    dims, origin, spacing = (6, 5, 4), (-10.0, 2.5, 0.75), (1.5, 2.0, 0.625)          # f32 values: the header holds them exactly
    values = rng.normal(size=(6 * 5 * 4, 3)).astype(np.float32)
    write_nifti(tmp_path / "f.nii.gz", dims, origin, spacing, values)
    (tmp_path / "c.json").write_text(json.dumps({"transforms": [{"type": "frogDisplacementField", "file": "f.nii.gz"}]}))
    links = read_transform(tmp_path / "c.json")
    assert len(links) == 1 and links[0].kind == FIELD == 3
    assert links[0].dims == dims and links[0].origin == origin and links[0].spacing == spacing
    assert np.array_equal(links[0].coeffs, values)
    status = C.c_int(-1)
    h = lib.frog_transform_read(str(tmp_path / "c.json").encode(), C.byref(status))
    assert h and status.value == 0 and lib.frog_transform_num_links(h) == 1
    l = lib.frog_transform_links(h)[0]
    assert l.type == 3 and tuple(l.dims) == dims and tuple(l.origin) == origin and tuple(l.spacing) == spacing
    assert np.array_equal(np.ctypeslib.as_array(l.coeffs, shape=(120, 3)), values)
    lib.frog_transform_free(h)


def test_mixed_entries_keep_their_order_and_old_files_parse_as_before(tmp_path):
    lib = _abi.host_lib()
    rng = np.random.default_rng(12)
    M = np.eye(4); M[0, 0] = 1.1; M[:3, 3] = [3, -2, 1]
    ldims, lorigin, lspacing = (4, 5, 6), (1.5, -2.0, 3.25), (10.0, 12.5, 8.0)
    c0 = rng.normal(size=(120, 3)).astype(np.float32); c1 = rng.normal(size=(120, 3)).astype(np.float32)
    fdims, forigin, fspacing = (3, 1, 5), (0.0, 4.0, -8.0), (2.0, 1.0, 0.5)
    fv = rng.normal(size=(15, 3)).astype(np.float32)
    write_nifti(tmp_path / "m.json.1.nii.gz", ldims, lorigin, lspacing, c1)
    write_nifti(tmp_path / "field.nii", fdims, forigin, fspacing, fv)
    inline = {"type": "vtkBSplineTransform", "dimensions": list(ldims), "origin": list(lorigin), "spacing": list(lspacing), "coeffs": c0.ravel().tolist()}
    entries = [{"type": "frogDisplacementField", "file": "field.nii"},
               {"type": "vtkMatrixToLinearTransform", "matrix": M.ravel().tolist()},
               inline,
               {"type": "frogDisplacementField", "file": "field.nii"},
               {"type": "vtkBSplineTransform", "file": "m.json.1.nii.gz"}]
    (tmp_path / "m.json").write_text(json.dumps({"transforms": entries}))
    (tmp_path / "old.json").write_text(json.dumps({"transforms": [entries[1], entries[2], entries[4]]}))
    kinds = [FIELD, LINEAR, BSPLINE, FIELD, BSPLINE]
    links = read_transform(tmp_path / "m.json")
    assert [l.kind for l in links] == kinds
    status = C.c_int(-1)
    h = lib.frog_transform_read(str(tmp_path / "m.json").encode(), C.byref(status))
    assert h and status.value == 0 and lib.frog_transform_num_links(h) == 5
    native = lib.frog_transform_links(h)
    assert [native[k].type for k in range(5)] == kinds
    for k, (dims, co) in enumerate([(fdims, fv), (None, None), (ldims, c0), (fdims, fv), (ldims, c1)]):
        if dims is None:
            assert np.array_equal(links[k].matrix, M) and np.array_equal(np.array(native[k].matrix[:]).reshape(4, 4), M)
            continue
        assert links[k].dims == dims == tuple(native[k].dims)
        assert np.array_equal(links[k].coeffs, co)
        assert np.array_equal(np.ctypeslib.as_array(native[k].coeffs, shape=(len(co), 3)), co)
    assert links[0].origin == forigin == tuple(native[0].origin) and links[0].spacing == fspacing == tuple(native[0].spacing)
    lib.frog_transform_free(h)
    # a file without the new entry gives the links it gave before: the same three, in order
    old = read_transform(tmp_path / "old.json")
    assert [l.kind for l in old] == [LINEAR, BSPLINE, BSPLINE]
    assert np.array_equal(old[1].coeffs, c0) and np.array_equal(old[2].coeffs, c1) and old[2].dims == ldims
    h = lib.frog_transform_read(str(tmp_path / "old.json").encode(), C.byref(status))
    assert h and [lib.frog_transform_links(h)[k].type for k in range(lib.frog_transform_num_links(h))] == [0, 1, 1]
    lib.frog_transform_free(h)


def test_missing_or_malformed_field_file_is_an_error(tmp_path):
    lib = _abi.host_lib()
    status = C.c_int(-1)
    (tmp_path / "c.json").write_text(json.dumps({"transforms": [{"type": "frogDisplacementField", "file": "absent.nii.gz"}]}))
    assert not lib.frog_transform_read(str(tmp_path / "c.json").encode(), C.byref(status)) and status.value == _abi.FROG_E_IO
    with pytest.raises(OSError):
        read_transform(tmp_path / "c.json")
    (tmp_path / "nofile.json").write_text(json.dumps({"transforms": [{"type": "frogDisplacementField"}]}))
    assert not lib.frog_transform_read(str(tmp_path / "nofile.json").encode(), C.byref(status)) and status.value == _abi.FROG_E_INVALID
    with pytest.raises(KeyError):
        read_transform(tmp_path / "nofile.json")
    # one component is a determinant map, not a field
    write_nifti(tmp_path / "j.nii.gz", (3, 3, 3), (0, 0, 0), (1, 1, 1), np.zeros(27, np.float32))
    (tmp_path / "j.json").write_text(json.dumps({"transforms": [{"type": "frogDisplacementField", "file": "j.nii.gz"}]}))
    assert not lib.frog_transform_read(str(tmp_path / "j.json").encode(), C.byref(status)) and status.value == _abi.FROG_E_INVALID
    with pytest.raises(ValueError):
        read_transform(tmp_path / "j.json")


def test_a_field_link_is_not_inverted():
    lib = _abi.hip_lib()
    field = Link.field((2, 3, 4), (0, 0, 0), (1, 1, 1), np.zeros((4, 3, 2, 3), np.float32))        # the (nz, ny, nx, 3) shape
    assert field.kind == FIELD and field.coeffs.shape == (24, 3)
    with pytest.raises(ValueError):
        Link.field((2, 3, 4), (0, 0, 0), (1, 1, 1), np.zeros((23, 3), np.float32))
    for links in ([field], smooth_chain() + [field], [field] + smooth_chain()):
        with pytest.raises(RuntimeError, match="no inverse form"):
            invert(links)
        src = (_abi.FrogChainLink * len(links))(*[l.view() for l in links])
        dst = (_abi.FrogChainLink * len(links))()
        assert lib.frog_chain_invert_links(src, len(links), dst) == _abi.FROG_E_INVALID
        assert b"field" in lib.frog_last_error()
    # chains without one: what they gave before
    links = smooth_chain()
    inv = invert(links)
    assert [l.kind for l in inv] == [BSPLINE_INVERSE, LINEAR]
    assert np.allclose(inv[1].matrix @ links[0].matrix, np.eye(4), atol=1e-13) and np.array_equal(inv[0].coeffs, links[1].coeffs)
    assert [l.kind for l in invert(inv)] == [LINEAR, BSPLINE]


def test_sample_refuses_a_null_chain_before_any_device_use():
    lib = _abi.hip_lib()
    o = (C.c_double * 3)(0, 0, 0); s = (C.c_double * 3)(1, 1, 1); d = (C.c_uint32 * 3)(2, 2, 2)
    out = np.zeros(8, np.float32)
    assert lib.frog_chain_sample(None, o, s, d, 6, None, out.ctypes.data) == _abi.FROG_E_INVALID
    assert b"frog_chain_sample" in lib.frog_last_error()


def test_transform_field_usage_and_argument_errors(tmp_path):
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and r.stdout.startswith("Usage : TransformField reference")
    for flag in ("-t", "-ti", "-s", "-o", "-j", "-w"):
        assert flag + " " in r.stdout
    write_nifti(tmp_path / "vol.nii.gz", (4, 4, 4), (0, 0, 0), (1, 1, 1), np.zeros(64, np.float32))
    r = subprocess.run([EXE, "vol.nii.gz"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "Error : one of -o and -j is needed" in r.stdout
    r = subprocess.run([EXE, "vol.nii.gz", "-j", "j.nii.gz", "-w", "c.json"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "Error : -w needs the field file of -o" in r.stdout
    r = subprocess.run([EXE, "vol.nii.gz", "-t", "absent.json", "-o", "f.nii.gz"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "Error : cannot read transform absent.json" in r.stdout
    r = subprocess.run([EXE, "absent.nii.gz", "-o", "f.nii.gz"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "Error : cannot read the grid of absent.nii.gz" in r.stdout
    assert not (tmp_path / "f.nii.gz").exists() and not (tmp_path / "c.json").exists()
