"""frog_chain_sample and the FROG_T_FIELD link (frog_amd/csrc/device/chain.hip) restated in NumPy f64, operation for operation.

Every step is a correctly rounded IEEE f64 operation on both sides (the device is built with -ffp-contract=off
-fno-fast-math), so the device's output must equal this one bit for bit:
    node        p = o + i * s
    linear link q_r = m0 * p0 + m1 * p1 + m2 * p2 + m3 (left to right);  J = the 3x3 block
    chain       A = I;  per link A <- J A with B[r][c] = J[r][0] * A[0][c] + J[r][1] * A[1][c] + J[r][2] * A[2][c]
    determinant A00 * (A11 * A22 - A12 * A21) - A01 * (A10 * A22 - A12 * A20) + A02 * (A10 * A21 - A11 * A20)
    field link  per axis c = (p - origin) / spacing clamped to [0, dims - 1], cell f0 = min(floor(c), dims - 2) (0 where
                dims == 1), f = c - f0, r = 1 - f;  d = rz * (ry * (rx * a + fx * b) + fy * (rx * c + fx * d)) + fz * (...)
                over the eight f32 nodes widened to f64;  q = p + d;  J = I + dd/dp of that interpolant, the column of a
                clamped axis (or one with a single node) zero."""
import numpy as np

from frog_amd.chain import FIELD, LINEAR

F8 = np.float64


def grid_nodes(origin, spacing, dims):
    """(p0, p1, p2), each of shape dims[::-1]: the nodes o + i * s, x fastest."""
    nx, ny, nz = (int(v) for v in dims)
    idx = (np.arange(nx, dtype=F8)[None, None, :], np.arange(ny, dtype=F8)[None, :, None], np.arange(nz, dtype=F8)[:, None, None])
    return [np.broadcast_to(F8(origin[a]) + idx[a] * F8(spacing[a]), (nz, ny, nx)) for a in range(3)]


def node_list(origin, spacing, dims):
    """The same nodes as an (N, 3) array in the order of the outputs."""
    return np.stack([p.ravel() for p in grid_nodes(origin, spacing, dims)], -1)


def determinant(A):
    return A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) \
        + A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0])


def affine_sample(links, origin, spacing, dims):
    """What Chain(links).sample(origin, spacing, dims, dtype=np.float64) returns for a chain of linear links."""
    node = grid_nodes(origin, spacing, dims)
    p = node
    A = [[F8(1.0 if r == c else 0.0) for c in range(3)] for r in range(3)]
    for link in links:
        if link.kind != LINEAR:
            raise ValueError("the restatement covers linear links only")
        m = link.matrix
        p = [m[r, 0] * p[0] + m[r, 1] * p[1] + m[r, 2] * p[2] + m[r, 3] for r in range(3)]
        A = [[m[r, 0] * A[0][c] + m[r, 1] * A[1][c] + m[r, 2] * A[2][c] for c in range(3)] for r in range(3)]
    disp = np.stack([p[r] - node[r] for r in range(3)], -1)
    return disp, np.full(node[0].shape, determinant(A), F8)


def field_apply(link, points, jacobian=False):
    """What Chain([link]).apply(points) returns for a field link; with jacobian=True also the (N, 3, 3) Jacobians."""
    if link.kind != FIELD:
        raise ValueError("a field link expected")
    pts = np.ascontiguousarray(points, F8).reshape(-1, 3)
    nx, ny, nz = link.dims
    dims = (nx, ny, nz)
    values = link.coeffs.astype(F8)                                 # widened, exactly
    i0, i1, f, flat = [], [], [], []
    for k in range(3):
        last = dims[k] - 1
        raw = (pts[:, k] - F8(link.origin[k])) / F8(link.spacing[k])
        c = np.where(raw < 0.0, 0.0, np.where(raw > F8(last), F8(last), raw))
        safe = np.where(np.isnan(c), 0.0, c)
        cell = np.where(c < F8(last), np.floor(safe), F8(last - 1 if last > 0 else 0)).astype(np.int64)
        i0.append(cell)
        i1.append(cell + 1 if last > 0 else np.zeros_like(cell))
        f.append(c - cell.astype(F8))
        flat.append((raw < 0.0) | (raw > F8(last)) | (last == 0))

    def node(x, y, z):
        return values[x + nx * (y + ny * z)]                        # (N, 3)

    a, b = node(i0[0], i0[1], i0[2]), node(i1[0], i0[1], i0[2])
    c, d = node(i0[0], i1[1], i0[2]), node(i1[0], i1[1], i0[2])
    e, g = node(i0[0], i0[1], i1[2]), node(i1[0], i0[1], i1[2])
    h, m = node(i0[0], i1[1], i1[2]), node(i1[0], i1[1], i1[2])
    fx, fy, fz = (v[:, None] for v in f)
    rx, ry, rz = 1 - fx, 1 - fy, 1 - fz
    v = rz * (ry * (rx * a + fx * b) + fy * (rx * c + fx * d)) + fz * (ry * (rx * e + fx * g) + fy * (rx * h + fx * m))
    out = pts + v
    if not jacobian:
        return out
    gx = rz * (ry * (b - a) + fy * (d - c)) + fz * (ry * (g - e) + fy * (m - h))
    gy = rz * (rx * (c - a) + fx * (d - b)) + fz * (rx * (h - e) + fx * (m - g))
    gz = ry * (rx * (e - a) + fx * (g - b)) + fy * (rx * (h - c) + fx * (m - d))
    J = np.zeros((len(pts), 3, 3), F8)
    for col, grad in enumerate((gx, gy, gz)):
        J[:, :, col] = np.where(flat[col][:, None], 0.0, grad / F8(link.spacing[col]))
        J[:, col, col] = 1.0 + J[:, col, col]
    return out, J
