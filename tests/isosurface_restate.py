"""NumPy restatement of frog_isosurface_* (include/frog_chain.h): marching tetrahedra on the Kuhn decomposition of every grid
cell, to the bit.  It derives its own 6 x 16 table from the rule in the header and shares no code with the library;
tests/test_isosurface.py tests it against facts that do not come from either, tests/test_gpu_isosurface.py holds the device
to it byte for byte."""
import itertools

import numpy as np

LEVEL, LABEL = 0, 1
PERMS = list(itertools.permutations(range(3)))          # xyz, xzy, yxz, yzx, zxy, zyx
POPCOUNT = np.array([bin(i).count("1") for i in range(128)], np.int64)


def tet_corners(pi):
    """The four cube corners (x, y, z in 0..1) of tetrahedron pi: v0 = 0, v1 = v0 + e_pi0, v2 = v1 + e_pi1, v3 = (1, 1, 1)."""
    v = np.zeros((4, 3), np.int64)
    v[1, pi[0]] = 1
    v[2] = v[1]
    v[2, pi[1]] += 1
    v[3] = 1
    return v


def tet_rule(inside):
    """The triangles of one tetrahedron: each vertex the pair of tetrahedron vertex numbers of the edge it lies on."""
    ins = [q for q in range(4) if inside[q]]
    out = [q for q in range(4) if not inside[q]]
    if len(ins) in (0, 4):
        return []
    if len(ins) == 1:
        a, (b, c, d) = ins[0], out
        return [[(a, b), (a, c), (a, d)]]
    if len(ins) == 3:
        a, (b, c, d) = out[0], ins
        return [[(b, a), (c, a), (d, a)]]
    (a, b), (c, d) = ins, out
    return [[(a, c), (a, d), (b, d)], [(a, c), (b, d), (b, c)]]


def _build_table():
    """cell[config] = the cell's triangles in order, each three (owner corner, edge code) pairs."""
    cell = []
    for config in range(256):
        tris = []
        for pi in PERMS:
            v = tet_corners(pi)
            inside = [bool(config >> int(c[0] + 2 * c[1] + 4 * c[2]) & 1) for c in v]
            for tri in tet_rule(inside):
                mid = np.array([(v[p] + v[q]) / 2.0 for p, q in tri])
                normal = np.cross(mid[1] - mid[0], mid[2] - mid[0])
                out_mean = np.mean([v[q] for q in range(4) if not inside[q]], axis=0)
                in_mean = np.mean([v[q] for q in range(4) if inside[q]], axis=0)
                dot = float(normal @ (out_mean - in_mean))
                assert dot != 0.0
                if dot <= 0:
                    tri = [tri[0], tri[2], tri[1]]
                entry = []
                for p, q in tri:
                    lo, hi = v[min(p, q)], v[max(p, q)]
                    d = hi - lo
                    entry.append((int(lo[0] + 2 * lo[1] + 4 * lo[2]), int(d[0] + 2 * d[1] + 4 * d[2] - 1)))
                tris.append(entry)
        cell.append(tris)
    return cell


CELL = _build_table()
N_TRI = np.array([len(t) for t in CELL], np.int64)
TRI = np.zeros((256, 12, 3, 2), np.int64)
for _c, _t in enumerate(CELL):
    if _t:
        TRI[_c, :len(_t)] = np.array(_t)


def inside_of(volume, level=None, label=None):
    volume = np.asarray(volume)
    if (level is None) == (label is None):
        raise ValueError("one of level and label")
    if label is not None:
        if volume.dtype.kind not in "iu":
            raise ValueError("label mode needs an integer volume")
        return volume.astype(np.int64) == int(label)
    with np.errstate(invalid="ignore"):
        return volume.astype(np.float64) >= np.float64(level)


def isosurface(volume, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), level=None, label=None):
    """volume[z, y, x]; origin and spacing as (x, y, z).  Returns (xyz float32 [n, 3], triangles uint32 [m, 3])."""
    volume = np.asarray(volume)
    inside = inside_of(volume, level, label)
    nz, ny, nx = volume.shape
    empty = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32)
    if min(nx, ny, nz) < 2 or not inside.any():
        return empty
    n = nx * ny * nz
    steps = (1, nx, nx * ny)

    # one vertex per crossing edge; an edge belongs to its lower node
    cross = np.zeros((nz, ny, nx, 7), bool)
    for code in range(7):
        dx, dy, dz = (code + 1) & 1, (code + 1) >> 1 & 1, (code + 1) >> 2 & 1
        cross[:nz - dz, :ny - dy, :nx - dx, code] = inside[:nz - dz, :ny - dy, :nx - dx] != inside[dz:, dy:, dx:]
    cross = cross.reshape(n, 7)
    mask = (cross * (1 << np.arange(7))).sum(axis=1)
    count = cross.sum(axis=1)
    offset = np.cumsum(count) - count
    node, code = np.nonzero(cross)                      # ascending node, then ascending code
    delta = np.stack([(code + 1) & 1, (code + 1) >> 1 & 1, (code + 1) >> 2 & 1], axis=1)
    other = node + delta @ np.array(steps)
    index = np.stack([node % nx, node // nx % ny, node // (nx * ny)], axis=1)
    flat = volume.reshape(-1)
    if label is not None:
        t = np.full(len(node), 0.5)
    else:
        va, vb = flat[node].astype(np.float64), flat[other].astype(np.float64)
        with np.errstate(all="ignore"):
            t = (np.float64(level) - va) / (vb - va)
        t[~(np.isfinite(va) & np.isfinite(vb))] = 0.5
    o, s = np.asarray(origin, np.float64), np.asarray(spacing, np.float64)
    with np.errstate(all="ignore"):
        pa = o + index.astype(np.float64) * s
        pb = o + (index + delta).astype(np.float64) * s
        xyz = (pa + t[:, None] * (pb - pa)).astype(np.float32)

    # triangles by cell, tetrahedron and rule
    config = np.zeros((nz - 1, ny - 1, nx - 1), np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, c >> 1 & 1, c >> 2 & 1
        config |= inside[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx].astype(np.int64) << c
    config = config.reshape(-1)
    k, j, i = np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    cell_node = (i + nx * (j + ny * k)).reshape(-1)
    per_cell = N_TRI[config]
    which = np.repeat(np.arange(len(config)), per_cell)
    within = np.arange(per_cell.sum()) - np.repeat(np.cumsum(per_cell) - per_cell, per_cell)
    entry = TRI[config[which], within]                  # [m, 3, (corner, code)]
    corner_step = np.array([(c & 1) + nx * ((c >> 1 & 1) + ny * (c >> 2 & 1)) for c in range(8)])
    owner = cell_node[which][:, None] + corner_step[entry[..., 0]]
    triangles = offset[owner] + POPCOUNT[mask[owner] & ((1 << entry[..., 1]) - 1)]
    return xyz, triangles.astype(np.uint32)


# ---- facts about a triangle mesh, by index -----------------------------------------------------------------------------------

def directed_edges(triangles):
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def is_closed(triangles):
    """Every directed edge is used exactly once and its reverse exactly once."""
    e = directed_edges(triangles)
    if not len(e):
        return True
    key, rev = e[:, 0] << 32 | e[:, 1], e[:, 1] << 32 | e[:, 0]
    return len(np.unique(key)) == len(key) and np.array_equal(np.sort(key), np.sort(rev))


def signed_volume(xyz, triangles):
    p = np.asarray(xyz, np.float64)[np.asarray(triangles, np.int64).reshape(-1, 3)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def euler_characteristic(xyz, triangles):
    return len(xyz) - len(directed_edges(triangles)) // 2 + len(np.asarray(triangles).reshape(-1, 3))


# ---- the cases both test files use ---------------------------------------------------------------------------------------------

SPHERES = [     # dims (x, y, z), R, spacing, origin
    ((13, 11, 9), 3.3, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)),
    ((13, 11, 9), 3.3 * 0.7, (0.7, 1.1, 1.6), (-3.0, 5.0, 11.0)),
    ((25, 23, 21), 9.1 * 0.5, (0.5, 0.5, 0.5), (0.0, 0.0, 0.0)),
]


def sphere(dims, radius, spacing, origin):
    """f = R - |x - c| as f32 [z, y, x], c the grid's centre."""
    ax = [np.float64(origin[a]) + np.arange(dims[a], dtype=np.float64) * np.float64(spacing[a]) for a in range(3)]
    centre = np.array([(a[0] + a[-1]) / 2 for a in ax])
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    f = radius - np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)
    return f.astype(np.float32), centre


def cell_configuration(config):
    """A 4^3 grid of zeros whose central cell has the corners of `config` set to one."""
    v = np.zeros((4, 4, 4), np.uint8)
    for c in range(8):
        if config >> c & 1:
            v[1 + (c >> 2 & 1), 1 + (c >> 1 & 1), 1 + (c & 1)] = 1
    return v


def ties_block():
    """A 5^3 grid with a 3^3 block of ones whose centre voxel is 2: at level 1.0 every crossing has t = 0 or 1."""
    v = np.zeros((5, 5, 5), np.float32)
    v[1:4, 1:4, 1:4] = 1
    v[2, 2, 2] = 2
    return v
