"""Scalar volumes for the reslicing step (tools/VolumeTransform.cxx): NIfTI-1 and MetaImage files through the
host library's reader and writer (include/frog_host.h)."""
import ctypes as C

import numpy as np

from . import _abi


def read_volume(path):
    """(voxels[z, y, x], origin(x, y, z), spacing(x, y, z)) of a .nii/.nii.gz/.mhd/.mha file."""
    lib = _abi.host_lib()
    status = C.c_int()
    h = lib.frog_volume_read(str(path).encode(), C.byref(status))
    if not h:
        raise OSError(f"cannot read volume {path} (status {status.value})")
    try:
        v = _abi.FrogVolume()
        lib.frog_volume_view(h, C.byref(v))
        dt = np.dtype(_abi.FROG_V_DTYPES[v.dtype])
        n = v.dims[0] * v.dims[1] * v.dims[2]
        buf = (C.c_char * (n * dt.itemsize)).from_address(v.data)
        a = np.frombuffer(buf, dt).reshape(v.dims[2], v.dims[1], v.dims[0]).copy()
        return a, tuple(v.origin), tuple(v.spacing)
    finally:
        lib.frog_volume_free(h)


def write_volume(path, voxels, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0)):
    """voxels[z, y, x] to .mhd (+ .zraw beside it), .nii or .nii.gz."""
    a = np.ascontiguousarray(voxels)
    v = _abi.volume_view(a, origin, spacing)
    rc = _abi.host_lib().frog_volume_write(str(path).encode(), C.byref(v))
    if rc:
        raise OSError(f"cannot write volume {path} (status {rc})")


def bbox_grid(path, spacing):
    """DummyVolumeGenerator's grid over bbox.json's box (frog_bbox_grid): (dims(x, y, z), origin, spacing)."""
    v = _abi.FrogVolume()
    _abi.check(_abi.host_lib().frog_bbox_grid(str(path).encode(), float(spacing), C.byref(v)), "frog_bbox_grid")
    return tuple(v.dims), tuple(v.origin), tuple(v.spacing)


def _as_volume(item):
    """(voxels[z, y, x], origin, spacing) as read_volume returns it, or a bare array (origin 0, spacing 1)."""
    if isinstance(item, np.ndarray):
        return np.ascontiguousarray(item), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    a, o, s = item
    return np.ascontiguousarray(a), tuple(float(v) for v in o), tuple(float(v) for v in s)


class Average:
    """frog_average (include/frog_chain.h): n_images volumes added one by one on `grid` = (dims(x, y, z), origin, spacing),
    then the f32 mean and stdev of AverageVolumes.cxx."""

    def __init__(self, grid, n_images, device=0):
        self._lib = _abi.hip_lib()
        dims, origin, spacing = grid
        self.dims = tuple(int(d) for d in dims)
        self._grid = _abi.volume_view(None, origin, spacing, self.dims)
        self._h = C.c_void_p()
        _abi.check(self._lib.frog_average_create(C.byref(self._grid), int(n_images), int(device), C.byref(self._h)), "frog_average_create")

    def close(self):
        if self._h:
            self._lib.frog_average_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, volume, chain=None, interpolation=1, background=0.0, resliced=False):
        """Adds `volume` ((voxels, origin, spacing) or an array already on the grid when chain is None); with a chain
        (frog_amd.chain.Chain, grid space -> volume space) it is resliced first as Chain.reslice does.  resliced=True
        returns that volume (source dtype, shape dims[::-1])."""
        a, o, s = _as_volume(volume)
        src = _abi.volume_view(a, o, s)
        out, ov = None, None
        if resliced:
            out = np.empty(self.dims[::-1], a.dtype)
            ov = _abi.volume_view(out, tuple(self._grid.origin), tuple(self._grid.spacing))
        _abi.check(self._lib.frog_average_add(self._h, chain._h if chain is not None else None, C.byref(src), int(interpolation),
                                              float(background), C.byref(ov) if ov is not None else None), "frog_average_add")
        return out

    def finish(self):
        """(mean, stdev), float32 arrays of shape dims[::-1]."""
        mean = np.empty(self.dims[::-1], np.float32)
        stdev = np.empty_like(mean)
        _abi.check(self._lib.frog_average_finish(self._h, mean.ctypes.data_as(_abi.c_float_p), stdev.ctypes.data_as(_abi.c_float_p)),
                   "frog_average_finish")
        return mean, stdev


def average(volumes, chains=None, grid=None, interpolation=1, backgrounds=None, device=0):
    """Voxel-wise mean and stdev of a group on the device (tools/AverageVolumes.cxx; with `chains`, transform.sh's
    VolumeTransform + AverageVolumes).  `volumes`: (voxels[z, y, x], origin, spacing) tuples or arrays; `chains`: None (the
    volumes are on the grid already) or one frog_amd.chain.Chain per volume, mapping grid space to the volume's;
    `grid`: (dims(x, y, z), origin, spacing), default the first volume's; `backgrounds`: None (each volume's minimum, as
    VolumeTransform), a number or one per volume.  Returns float32 (mean, stdev), NaN where upstream's f32 variance
    rounds negative."""
    vols = [_as_volume(v) for v in volumes]
    if not vols:
        raise ValueError("no volumes")
    if chains is not None and len(chains) != len(vols):
        raise ValueError("one chain per volume expected")
    if grid is None:
        a, o, s = vols[0]
        grid = (a.shape[::-1], o, s)
    if backgrounds is None:
        backgrounds = [float(a.min()) for a, _, _ in vols]
    elif np.ndim(backgrounds) == 0:
        backgrounds = [float(backgrounds)] * len(vols)
    acc = Average(grid, len(vols), device)
    try:
        for k, v in enumerate(vols):
            acc.add(v, None if chains is None else chains[k], interpolation, backgrounds[k])
        return acc.finish()
    finally:
        acc.close()
