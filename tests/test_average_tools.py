"""The average-image tools without a device: bin/DummyVolumeGenerator (tools/DummyVolumeGenerator.cxx), frog_bbox_grid,
and the argument checks of frog_average_create / the average tools that come before any device use."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

from frog_amd import _abi
from frog_amd.volume import bbox_grid, read_volume

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _dummy(tmp_path, bbox, spacing):
    return subprocess.run([os.path.join(BIN, "DummyVolumeGenerator"), str(bbox), str(spacing)], cwd=tmp_path,
                          capture_output=True, text=True, timeout=60)


def _expected(bbox_path, spacing):
    lo, hi = json.load(open(bbox_path))["bbox"]
    return tuple(int(math.ceil((b - a) / spacing)) for a, b in zip(lo, hi)), tuple(float(v) for v in lo)


@pytest.mark.parametrize("source,spacing", [("frog", 2.0), ("frog", 3.7), ("hand", 2.0), ("hand", 0.75)])
def test_dummy_volume_generator_grid(tmp_path, source, spacing):
    if source == "frog":
        bbox = os.path.join(GOLDEN, "frog_bbox.json")          # as bin/frog wrote it (stats + bbox)
        assert "images" in json.load(open(bbox))
    else:                                                       # extents that are not multiples of the spacing
        bbox = tmp_path / "box.json"
        bbox.write_text(json.dumps({"bbox": [[-10.25, 3.0, -0.5], [31.0, 47.9, 20.1]]}))
    dims, origin = _expected(bbox, spacing)
    r = _dummy(tmp_path, bbox, spacing)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "dummy.zraw").exists()
    vox, o, s = read_volume(tmp_path / "dummy.mhd")
    assert vox.dtype == np.float32 and vox.shape == dims[::-1] and not vox.any()
    assert o == origin and s == (spacing,) * 3
    assert bbox_grid(bbox, spacing) == (dims, origin, (spacing,) * 3)


def test_dummy_volume_generator_errors(tmp_path):
    exe = os.path.join(BIN, "DummyVolumeGenerator")
    r = subprocess.run([exe, "only_one"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 254 and "Usage : DummyVolumeGenerator bbox.json spacing" in r.stdout
    for i, text in enumerate(['{"bbox": [[0, 0, 0]]}', '{"bbox": [[0, 0], [1, 1]]}', '{"box": [[0, 0, 0], [1, 1, 1]]}',
                              '{"bbox": [[0, 0, 0], [1, 1, 1]', '{"bbox": [[0, 0, 0], [0, 5, 5]]}', "not json"]):
        (tmp_path / f"bad{i}.json").write_text(text)
        r = _dummy(tmp_path, f"bad{i}.json", 1.0)
        assert r.returncode != 0, text
    (tmp_path / "ok.json").write_text('{"bbox": [[0, 0, 0], [4, 4, 4]]}')
    for spacing in ("0", "-1"):
        assert _dummy(tmp_path, "ok.json", spacing).returncode != 0
    assert _dummy(tmp_path, "missing.json", 1.0).returncode != 0
    assert not (tmp_path / "dummy.mhd").exists() and not (tmp_path / "dummy.zraw").exists()


def test_bbox_grid_rejects_bad_arguments(tmp_path):
    lib = _abi.host_lib()
    (tmp_path / "ok.json").write_text('{"bbox": [[0, 0, 0], [4, 4, 4]]}')
    (tmp_path / "bad.json").write_text('{"bbox": [[0, 0, 0], [4, "a", 4]]}')
    v = _abi.FrogVolume()
    ok = str(tmp_path / "ok.json").encode()
    assert lib.frog_bbox_grid(ok, 0.0, C.byref(v)) == _abi.FROG_E_INVALID
    assert lib.frog_bbox_grid(ok, -2.0, C.byref(v)) == _abi.FROG_E_INVALID
    assert lib.frog_bbox_grid(ok, float("nan"), C.byref(v)) == _abi.FROG_E_INVALID
    assert lib.frog_bbox_grid(str(tmp_path / "bad.json").encode(), 1.0, C.byref(v)) == _abi.FROG_E_INVALID
    assert lib.frog_bbox_grid(str(tmp_path / "none.json").encode(), 1.0, C.byref(v)) == _abi.FROG_E_INVALID
    assert lib.frog_bbox_grid(ok, 1.5, None) == _abi.FROG_E_INVALID
    assert lib.frog_bbox_grid(ok, 1.5, C.byref(v)) == _abi.FROG_OK
    assert tuple(v.dims) == (3, 3, 3) and v.dtype == _abi.FROG_V_DTYPES.index("float32") and not v.data


def test_average_create_checks_arguments_before_the_device():
    lib = _abi.hip_lib()
    h = C.c_void_p()
    g = _abi.FrogVolume()
    g.dims[:] = (4, 4, 4); g.spacing[:] = (1, 1, 1)
    assert lib.frog_average_create(None, 3, 0, C.byref(h)) == _abi.FROG_E_INVALID
    assert lib.frog_average_create(C.byref(g), 0, 0, C.byref(h)) == _abi.FROG_E_INVALID
    assert lib.frog_average_create(C.byref(g), 3, 0, None) == _abi.FROG_E_INVALID
    g.dims[:] = (4, 0, 4)
    assert lib.frog_average_create(C.byref(g), 3, 0, C.byref(h)) == _abi.FROG_E_INVALID
    g.dims[:] = (2048, 1024, 1025)                              # 2^31 + 2^21 voxels: refused before any launch
    assert lib.frog_average_create(C.byref(g), 3, 0, C.byref(h)) == _abi.FROG_E_INVALID
    assert b"2^31" in lib.frog_last_error()
    assert not h.value
    assert lib.frog_average_add(None, None, None, 1, 0.0, None) == _abi.FROG_E_INVALID
    assert lib.frog_average_finish(None, None, None) == _abi.FROG_E_INVALID
    lib.frog_average_destroy(None)
    if lib.frog_device_count() > 0:
        return                                                  # the NODEVICE answer is for hosts without a GPU
    g.dims[:] = (4, 4, 4)
    assert lib.frog_average_create(C.byref(g), 3, 0, C.byref(h)) == _abi.FROG_E_NODEVICE and not h.value
    assert b"no CPU fallback" in lib.frog_last_error()


def test_average_tools_usage_and_checks_without_a_device(tmp_path):
    r = subprocess.run([os.path.join(BIN, "AverageVolumes")], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Usage : AverageVolumes" in r.stdout
    exe = os.path.join(BIN, "AverageImage")
    r = subprocess.run([exe, "bbox.json", "2"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Usage : AverageImage" in r.stdout
    # a missing transform is named, and nothing is written (the check comes before the device is asked for)
    (tmp_path / "bbox.json").write_text('{"bbox": [[0, 0, 0], [8, 8, 8]]}')
    (tmp_path / "transforms").mkdir()
    (tmp_path / "transforms" / "0.json").write_text(json.dumps({"transforms": [
        {"type": "vtkMatrixToLinearTransform", "matrix": np.eye(4).ravel().tolist()}]}))
    r = subprocess.run([exe, "bbox.json", "2", "a.nii.gz", "b.nii.gz", "-o", "out"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "transforms/1.json" in r.stdout, r.stdout
    assert not (tmp_path / "out").exists()
    # every transform there, a volume missing: named, nothing written
    (tmp_path / "transforms" / "1.json").write_text((tmp_path / "transforms" / "0.json").read_text())
    r = subprocess.run([exe, "bbox.json", "2", "a.nii.gz", "b.nii.gz", "-o", "out"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "a.nii.gz" in r.stdout, r.stdout
    assert not (tmp_path / "out").exists()
