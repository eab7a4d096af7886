"""NumPy restatement of the mesh filters of include/frog_chain.h -- Taubin's lambda | mu smoothing on the vertex graph and
decimation by vertex clustering -- to the bit, vectorised.  It shares no code with the library; tests/test_mesh_filters.py
tests it against facts that do not come from it (a brute-force version among them), tests/test_gpu_mesh_filters.py holds the
device to it byte for byte.  Refusals (FROG_E_INVALID in the library) are ValueError here."""
import numpy as np

import isosurface_restate as IR

F4, F8, U4 = np.float32, np.float64, np.uint32
DEFAULTS = dict(iterations=20, lam=0.5, mu=-0.53, boundary=1)


def faces_arrays(faces):
    """(face_ptr int64 [m + 1], face_idx int64) of a 2-D index array or of a sequence of index sequences."""
    if isinstance(faces, np.ndarray) and faces.ndim == 2:
        m, k = faces.shape
        return np.arange(m + 1, dtype=np.int64) * k, faces.astype(np.int64).reshape(-1)
    rows = [np.asarray(f, np.int64).reshape(-1) for f in faces]
    ptr = np.zeros(len(rows) + 1, np.int64)
    if rows:
        ptr[1:] = np.cumsum([len(r) for r in rows])
    return ptr, (np.concatenate(rows) if rows else np.zeros(0, np.int64))


def face_edges(n, faces):
    """The faces' edges as (a, b) in face order, pairs of equal indices left out.  An index >= n: ValueError."""
    ptr, idx = faces_arrays(faces)
    if len(idx) and (idx.min() < 0 or idx.max() >= n):
        raise ValueError("face index out of range")
    face = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    j = np.arange(len(idx))
    after = np.where(j + 1 < ptr[face + 1], j + 1, ptr[face])      # the last index pairs with the first
    a, b = idx[j], idx[after]
    keep = a != b
    return a[keep], b[keep]


def neighbours(n, faces, boundary=1):
    """The CSR of N(v): (ptr int64 [n + 1], col int64), columns ascending inside a row."""
    if boundary not in (0, 1):
        raise ValueError("boundary 0 or 1")
    a, b = face_edges(n, faces)
    key = np.concatenate([a << 32 | b, b << 32 | a])                # {a, b} in whichever orientation, seen from both ends
    unique, times = np.unique(key, return_counts=True)
    row, col = unique >> 32, unique & 0xffffffff
    on_boundary = np.zeros(n, bool)
    on_boundary[row[times == 1]] = True
    keep = ~on_boundary[row] | ((times == 1) & bool(boundary))
    row, col = row[keep], col[keep]
    ptr = np.zeros(n + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(row, minlength=n))
    return ptr, col


def one_pass(x, ptr, col, f):
    """x' of one pass with factor f: float32 [n, 3] from float32 [n, 3]."""
    degree = np.diff(ptr)
    s = np.zeros((len(x), 3), F8)
    for k in range(int(degree.max()) if len(degree) else 0):        # the k-th neighbour of every row that has one: ascending order
        rows = np.nonzero(degree > k)[0]
        s[rows] = s[rows] + x[col[ptr[rows] + k]].astype(F8)
    moving = degree > 0
    out = x.copy()
    with np.errstate(all="ignore"):
        m = s[moving] / degree[moving].astype(F8)[:, None]
        own = x[moving].astype(F8)
        out[moving] = (own + F8(f) * (m - own)).astype(F4)
    return out


def smooth(xyz, faces, iterations=20, lam=0.5, mu=-0.53, boundary=1):
    x = np.array(xyz, F4).reshape(-1, 3)
    if not (np.isfinite(lam) and np.isfinite(mu)):
        raise ValueError("lambda and mu are finite")
    ptr, col = neighbours(len(x), faces, boundary)
    if iterations == 0 or (lam == 0 and mu == 0):
        return x
    for _ in range(iterations):
        x = one_pass(x, ptr, col, lam)
        x = one_pass(x, ptr, col, mu)
    return x


def cluster(xyz, triangles, cell):
    """(xyz float32 [k, 3], triangles uint32 [m', 3], cluster_of uint32 [n])."""
    x = np.ascontiguousarray(xyz, F4).reshape(-1, 3)
    t = np.asarray(triangles)
    if t.size and (t.ndim != 2 or t.shape[1] != 3):
        raise ValueError("triangles only")
    t = t.astype(np.int64).reshape(-1, 3)
    cell = F8(cell)
    if not (np.isfinite(cell) and cell > 0):
        raise ValueError("the cell is a finite size > 0")
    if len(t) and (t.min() < 0 or t.max() >= len(x)):
        raise ValueError("face index out of range")
    if not len(x):
        return np.zeros((0, 3), F4), np.zeros((0, 3), U4), np.zeros(0, U4)
    if not np.isfinite(x).all():
        raise ValueError("a coordinate is not finite")
    lo = x.min(axis=0)
    with np.errstate(over="ignore"):
        q = np.floor((x.astype(F8) - lo.astype(F8)) / cell)
    if not (q.max() < 2.0 ** 21):
        raise ValueError("more than 2^21 cells on an axis")
    c = q.astype(np.int64)
    count = c.max(axis=0) + 1
    key = (c[:, 2] * count[1] + c[:, 1]) * count[0] + c[:, 0]
    unique, cluster_of = np.unique(key, return_inverse=True)
    cluster_of = cluster_of.reshape(-1)
    members = np.argsort(cluster_of, kind="stable")                 # by cluster, ascending old index inside one
    size = np.bincount(cluster_of, minlength=len(unique))
    first = np.cumsum(size) - size
    s = np.zeros((len(unique), 3), F8)
    xd = x.astype(F8)
    small = 64
    for k in range(int(min(size.max(), small))):                    # the k-th member of every cluster that has one
        rows = np.nonzero((size > k) & (size <= small))[0]
        s[rows] = s[rows] + xd[members[first[rows] + k]]
    for row in np.nonzero(size > small)[0]:                         # a long cluster: a running sum is sequential, from +0
        run = np.concatenate([np.zeros((1, 3), F8), xd[members[first[row]:first[row] + size[row]]]])
        s[row] = np.cumsum(run, axis=0)[-1]
    new_xyz = (s / size.astype(F8)[:, None]).astype(F4)
    image = cluster_of[t]
    keep = (image[:, 0] != image[:, 1]) & (image[:, 1] != image[:, 2]) & (image[:, 2] != image[:, 0])
    return new_xyz, image[keep].astype(U4), cluster_of.astype(U4)


# ---- the cases both test files use ---------------------------------------------------------------------------------------------

def blocky_ball():
    """The label surface of a voxel ball: 3 830 vertices on edge midpoints, 7 656 triangles, closed, Euler characteristic 2."""
    f, centre = IR.sphere((25, 23, 21), 8.2, (1, 1, 1), (0, 0, 0))
    xyz, tri = IR.isosurface((f >= 0).astype(np.uint8), label=1)
    return xyz, tri, centre


def octahedron(radius=8.0):
    xyz = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F4) * F4(radius)
    tri = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], U4)
    return xyz, tri


def grid(nx=6, ny=6, noise=0.0, seed=3):
    """nx x ny vertices on the integers (z = 0, or noise in z), each square cut along the same diagonal."""
    j, i = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    xyz = np.stack([i.reshape(-1), j.reshape(-1), np.zeros(nx * ny)], axis=1).astype(F4)
    if noise:
        xyz[:, 2] = (np.random.default_rng(seed).standard_normal(nx * ny) * noise).astype(F4)
    v = (i + nx * j)[:-1, :-1].reshape(-1)
    tri = np.concatenate([np.stack([v, v + 1, v + nx + 1], axis=1), np.stack([v, v + nx + 1, v + nx], axis=1)])
    return xyz, tri.astype(U4)


def fan(rim=300, seed=5):
    """A closed fan: hub 0 with `rim` neighbours, more than a wavefront and more than a block's width."""
    rng = np.random.default_rng(seed)
    angle = 2 * np.pi * np.arange(rim) / rim
    xyz = np.zeros((rim + 1, 3), F4)
    xyz[1:, 0], xyz[1:, 1] = 10 * np.cos(angle), 10 * np.sin(angle)
    xyz += (rng.standard_normal(xyz.shape) * 0.3).astype(F4)
    k = np.arange(rim)
    return xyz, np.stack([np.zeros(rim, np.int64), 1 + k, 1 + (k + 1) % rim], axis=1).astype(U4)


def strip(n, seed=7):
    """A chain of n - 2 triangles over n vertices (none for n < 3), alternating so that the orientation is consistent."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    xyz = np.stack([i * 0.5, (i % 2) * 1.0, np.zeros(n)], axis=1).astype(F4) + (rng.standard_normal((n, 3)) * 0.1).astype(F4)
    k = np.arange(max(n - 2, 0))
    tri = np.stack([k, np.where(k % 2 == 0, k + 1, k + 2), np.where(k % 2 == 0, k + 2, k + 1)], axis=1)
    return xyz, tri.astype(U4).reshape(-1, 3)


def far_apart():
    """Three vertices about 2^20 cells of size 1 apart on every axis (cells 0, 2^20 and 2^21 - 1: the keys pass 2^32 and the
    grid has the 2^21 cells per axis that are the most accepted), and a fourth in the second one's cell."""
    step, top = 2.0 ** 20, 2.0 ** 21 - 1
    xyz = np.array([[0, 0, 0], [step, step, step], [top, top, top], [step, step, step + 0.25]], F4)
    return xyz, np.array([[0, 1, 2], [2, 1, 0], [0, 1, 3]], U4)


def radial_stdev(xyz, centre):
    return float(np.linalg.norm(np.asarray(xyz, F8) - centre, axis=1).std())


def edges_balanced(triangles):
    """Every directed edge occurs as often as its reverse."""
    e = IR.directed_edges(triangles)
    if not len(e):
        return True
    return np.array_equal(np.sort(e[:, 0] << 32 | e[:, 1]), np.sort(e[:, 1] << 32 | e[:, 0]))
