"""Surface meshes: files (include/frog_host.h: frog_mesh_*), points through a transform chain in f32
(frog_chain_apply_f32, tools/MeshTransform.cxx) and iso-surface extraction on the GPU (frog_isosurface_*,
include/frog_chain.h: marching tetrahedra on the Kuhn decomposition) -- the ctypes layer."""
import ctypes as C
import os

import numpy as np

from . import _abi
from ._abi import check
from .volume import _as_volume


class MeshError(RuntimeError):
    def __init__(self, code, where):
        msg = _abi.host_lib().frog_mesh_last_error()
        super().__init__(f"{where}: status {code}: {msg.decode() if msg else ''}")
        self.code = code


def _faces_arrays(faces):
    """(face_ptr uint32 [m + 1], face_idx uint32) of a 2-D index array or of a sequence of index sequences."""
    if isinstance(faces, np.ndarray) and faces.ndim == 2:
        m, k = faces.shape
        return np.arange(m + 1, dtype=np.uint32) * np.uint32(k), np.ascontiguousarray(faces, np.uint32).reshape(-1)
    rows = [np.asarray(f, np.uint32).reshape(-1) for f in faces]
    ptr = np.zeros(len(rows) + 1, np.uint32)
    if rows:
        ptr[1:] = np.cumsum([len(r) for r in rows])
    return ptr, (np.concatenate(rows) if rows else np.zeros(0, np.uint32))


def read_mesh(path):
    """(xyz float32 [n, 3], faces) of an .obj, .ply, .stl or legacy .vtk file.  faces is a uint32 array [m, k] when every
    face has k points (triangles: [m, 3]; no faces: [0, 3]), otherwise a list of m uint32 arrays.  Point normals, texture
    coordinates and colours are not carried."""
    lib = _abi.host_lib()
    status = C.c_int()
    h = lib.frog_mesh_read(os.fsencode(path), C.byref(status))
    if not h:
        raise MeshError(status.value, "frog_mesh_read")
    try:
        v = _abi.FrogMesh()
        lib.frog_mesh_view(h, C.byref(v))
        n, m = int(v.n_points), int(v.n_faces)
        xyz = np.ctypeslib.as_array(v.xyz, (n, 3)).copy() if n else np.zeros((0, 3), np.float32)
        ptr = np.ctypeslib.as_array(v.face_ptr, (m + 1,)).copy()
        idx = np.ctypeslib.as_array(v.face_idx, (int(ptr[-1]),)).copy() if ptr[-1] else np.zeros(0, np.uint32)
    finally:
        lib.frog_mesh_free(h)
    sizes = np.diff(ptr)
    if m == 0:
        return xyz, np.zeros((0, 3), np.uint32)
    if (sizes == sizes[0]).all():
        return xyz, idx.reshape(m, int(sizes[0]))
    return xyz, [idx[ptr[f]:ptr[f + 1]] for f in range(m)]


def write_mesh(path, xyz, faces):
    """Writes points and faces (as read_mesh returns them) to .obj, .ply, .stl, .vtk or .vtp, chosen by the extension."""
    p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    ptr, idx = _faces_arrays(faces)
    v = _abi.FrogMesh(len(p), p.ctypes.data_as(_abi.c_float_p), len(ptr) - 1, ptr.ctypes.data_as(_abi.c_u32_p),
                      idx.ctypes.data_as(_abi.c_u32_p))
    code = _abi.host_lib().frog_mesh_write(os.fsencode(path), C.byref(v))
    if code != _abi.FROG_OK:
        raise MeshError(code, "frog_mesh_write")


def transform_points(chain, xyz):
    """float32(chain(float64(xyz))) on the GPU (frog_chain_apply_f32): what bin/MeshTransform does to a mesh's points."""
    p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    out = np.empty_like(p)
    check(_abi.hip_lib().frog_chain_apply_f32(chain._h, p.ctypes.data_as(_abi.c_float_p), out.ctypes.data_as(_abi.c_float_p), len(p)),
          "frog_chain_apply_f32")
    return out


SMOOTH_DEFAULTS = {"iterations": 20, "lam": 0.5, "mu": -0.53, "boundary": 1}


def smooth(xyz, faces, iterations=20, lam=0.5, mu=-0.53, boundary=1, device=0):
    """Taubin's lambda | mu smoothing of a mesh's points on the GPU (frog_mesh_smooth, include/frog_chain.h): `iterations`
    times a pass with `lam`, then one with `mu`; polygons of any size; boundary=1 lets a border slide along itself, 0 pins
    it.  Returns the new points (float32 [n, 3]); the faces are not touched."""
    p = np.array(xyz, np.float32, order="C").reshape(-1, 3)
    ptr, idx = _faces_arrays(faces)
    check(_abi.hip_lib().frog_mesh_smooth(p.ctypes.data_as(_abi.c_float_p), len(p), ptr.ctypes.data_as(_abi.c_u32_p),
                                          idx.ctypes.data_as(_abi.c_u32_p), len(ptr) - 1, int(iterations), float(lam), float(mu),
                                          int(boundary), int(device)), "frog_mesh_smooth")
    return p


def _get(lib, h, n, m):
    xyz, tri = np.empty((n, 3), np.float32), np.empty((m, 3), np.uint32)
    check(lib.frog_isosurface_get(h, xyz.ctypes.data_as(_abi.c_float_p), tri.ctypes.data_as(_abi.c_u32_p)), "frog_isosurface_get")
    return xyz, tri


def _cluster(lib, h, cell, n_old):
    """frog_isosurface_cluster on a handle: (n, m, cluster_of)."""
    n, m = C.c_uint32(), C.c_uint32()
    cluster_of = np.empty(n_old, np.uint32)
    check(lib.frog_isosurface_cluster(h, float(cell), C.byref(n), C.byref(m), cluster_of.ctypes.data_as(_abi.c_u32_p)),
          "frog_isosurface_cluster")
    return n.value, m.value, cluster_of


def cluster(xyz, triangles, cell, device=0):
    """Decimation by vertex clustering on the GPU (frog_isosurface_upload + frog_isosurface_cluster): one vertex per occupied
    cell of size `cell`, at the mean of its members.  Returns (xyz float32 [k, 3], triangles uint32 [m', 3], cluster_of
    uint32 [n]): the new index of every old vertex."""
    lib = _abi.hip_lib()
    p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    t = np.asarray(triangles)
    if t.size and (t.ndim != 2 or t.shape[1] != 3):
        raise ValueError("cluster takes triangles")
    t = np.ascontiguousarray(t, np.uint32).reshape(-1, 3)
    h = C.c_void_p()
    check(lib.frog_isosurface_upload(p.ctypes.data_as(_abi.c_float_p), len(p), t.ctypes.data_as(_abi.c_u32_p), len(t), int(device),
                                     C.byref(h)), "frog_isosurface_upload")
    try:
        n, m, cluster_of = _cluster(lib, h, cell, len(p))
        return _get(lib, h, n, m) + (cluster_of,)
    finally:
        lib.frog_isosurface_destroy(h)


def isosurface(volume, level=None, label=None, chain=None, device=0, smooth=None, cell=None):
    """The iso-surface of `volume` -- (voxels[z, y, x], origin(x, y, z), spacing(x, y, z)) or a bare array -- where
    voxel >= level, or of a label map where voxel == label: (xyz float32 [n, 3], triangles uint32 [m, 3]), welded,
    normals pointing out, in the deterministic order of include/frog_chain.h.  `smooth` (True for the defaults, an iteration
    count, or a dict of smooth()'s iterations, lam, mu, boundary) and `cell` (a cluster size) filter the mesh on the device,
    in that order (frog_isosurface_smooth, frog_isosurface_cluster).  With `chain` the vertices then go through it on the
    device before the copy back (frog_isosurface_apply)."""
    if (level is None) == (label is None):
        raise ValueError("one of level and label")
    lib = _abi.hip_lib()
    a, origin, spacing = _as_volume(volume)
    v = _abi.volume_view(a, origin, spacing)
    h, n, m = C.c_void_p(), C.c_uint32(), C.c_uint32()
    mode = _abi.FROG_ISO_LEVEL if label is None else _abi.FROG_ISO_LABEL
    check(lib.frog_isosurface_create(C.byref(v), mode, 0.0 if level is None else float(level), 0 if label is None else int(label),
                                     int(device), C.byref(h), C.byref(n), C.byref(m)), "frog_isosurface_create")
    try:
        n, m = n.value, m.value
        if smooth is not None and smooth is not False:
            how = dict(SMOOTH_DEFAULTS)
            if isinstance(smooth, dict):
                how.update(smooth)
            elif smooth is not True:
                how["iterations"] = int(smooth)
            check(lib.frog_isosurface_smooth(h, int(how["iterations"]), float(how["lam"]), float(how["mu"]), int(how["boundary"])),
                  "frog_isosurface_smooth")
        if cell is not None:
            n, m, _ = _cluster(lib, h, cell, n)
        if chain is not None:
            check(lib.frog_isosurface_apply(h, chain._h), "frog_isosurface_apply")
        xyz, tri = _get(lib, h, n, m)
    finally:
        lib.frog_isosurface_destroy(h)
    return xyz, tri
