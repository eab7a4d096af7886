"""reslice_voxel (frog_amd/csrc/device/chain.hip) restated in NumPy f64, operation for operation, for chains of linear links.

Every step is a correctly rounded IEEE f64 operation on both sides (the device is built with -ffp-contract=off
-fno-fast-math), so the device's output must equal this one bit for bit:
    p = oo + i * os;  q_r = m0 * p0 + m1 * p1 + m2 * p2 + m3 (left to right) per link;  c = (p - so) / ss
    inside: -0.5 <= c <= dims - 0.5 on every axis, else the background
    nearest: the voxel floor(c + 0.5);  linear: rz * (ry * (rx * a + fx * b) + fy * (...)) + fz * (...), taps clamped
    integers: floor(v + 0.5) clamped to the type's range;  floats: a plain cast."""
import numpy as np

from frog_amd.chain import LINEAR

F8 = np.float64


def to_voxel(v, dtype):
    dt = np.dtype(dtype)
    if dt.kind in "iu":
        info = np.iinfo(dt)
        lo, hi = F8(info.min), F8(info.max)
        x = np.floor(v + 0.5)
        return np.where(x < lo, lo, np.where(x > hi, hi, x)).astype(dt)
    return np.asarray(v, F8).astype(dt)


def sample_positions(links, out_dims, out_origin, out_spacing):
    """Positions (p0, p1, p2) of the output voxels after the chain, each an array of shape out_dims[::-1]."""
    nx, ny, nz = (int(v) for v in out_dims)
    shape = (nz, ny, nx)
    idx = (np.arange(nx, dtype=F8)[None, None, :], np.arange(ny, dtype=F8)[None, :, None], np.arange(nz, dtype=F8)[:, None, None])
    p = [np.broadcast_to(F8(out_origin[a]) + idx[a] * F8(out_spacing[a]), shape) for a in range(3)]
    for link in links:
        if link.kind != LINEAR:
            raise ValueError("the restatement covers linear links only")
        m = link.matrix
        p = [m[r, 0] * p[0] + m[r, 1] * p[1] + m[r, 2] * p[2] + m[r, 3] for r in range(3)]
    return p


def reslice(links, volume, origin, spacing, out_dims, out_origin, out_spacing, interpolation=1, background=0.0):
    """What Chain(links).reslice(volume, origin, spacing, out_dims, out_origin, out_spacing, interpolation, background) returns."""
    vol = np.ascontiguousarray(volume)
    sz, sy, sx = vol.shape
    dims = (sx, sy, sz)
    p = sample_positions(links, out_dims, out_origin, out_spacing)
    c = [(p[a] - F8(origin[a])) / F8(spacing[a]) for a in range(3)]
    inside = np.ones(p[0].shape, bool)
    for a in range(3):
        inside &= (c[a] >= -0.5) & (c[a] <= F8(dims[a]) - 0.5)
    c = [np.where(inside, c[a], 0.0) for a in range(3)]          # outside: any in-range index, the value is not used
    flat = vol.ravel().astype(F8)

    def at(x, y, z):
        x = np.clip(x, 0, sx - 1); y = np.clip(y, 0, sy - 1); z = np.clip(z, 0, sz - 1)
        return flat[x + sx * (y + sy * z)]

    if not interpolation:
        v = at(*[np.floor(c[a] + 0.5).astype(np.int64) for a in range(3)])
    else:
        f = [np.floor(c[a]) for a in range(3)]
        x0, y0, z0 = (t.astype(np.int64) for t in f)
        fx, fy, fz = (c[a] - f[a] for a in range(3))
        rx, ry, rz = 1 - fx, 1 - fy, 1 - fz
        v = rz * (ry * (rx * at(x0, y0, z0) + fx * at(x0 + 1, y0, z0)) + fy * (rx * at(x0, y0 + 1, z0) + fx * at(x0 + 1, y0 + 1, z0))) \
            + fz * (ry * (rx * at(x0, y0, z0 + 1) + fx * at(x0 + 1, y0, z0 + 1)) + fy * (rx * at(x0, y0 + 1, z0 + 1) + fx * at(x0 + 1, y0 + 1, z0 + 1)))
    return to_voxel(np.where(inside, v, F8(background)), vol.dtype)


def extreme_volume(dtype, shape, rng, huge_floats=True):
    """A volume that holds its type's edges: min and max of the integer types (u32 mostly above 2^31, i32 mostly within
    1000 of +-2^31, ramps across 2^24 for both), f64 values that need more than 24 significand bits, f32 subnormals (and,
    with huge_floats, +-FLT_MAX and f64 values near 1e300)."""
    dt = np.dtype(dtype)
    n = int(np.prod(shape))
    if dt.kind in "iu":
        info = np.iinfo(dt)
        v = rng.integers(int(info.min), int(info.max), n, dtype=np.int64 if dt != np.uint32 else np.uint64, endpoint=True)
        if dt == np.uint32:
            v[::2] = rng.integers(2 ** 31, 2 ** 32, len(v[::2]), dtype=np.uint64)
        if dt == np.int32:
            v[::3] = rng.integers(2 ** 31 - 1000, 2 ** 31, len(v[::3]))
            v[1::3] = rng.integers(-2 ** 31, -2 ** 31 + 1000, len(v[1::3]))
        if dt.itemsize == 4:
            v[5::17] = rng.integers(2 ** 24 - 4, 2 ** 24 + 4, len(v[5::17]))
        v = v.astype(dt)
        v[::7] = info.min
        v[3::7] = info.max
    elif dt == np.float32:
        v = rng.normal(0, 1e3, n).astype(np.float32)
        v[::5] = (rng.uniform(-1, 1, len(v[::5])) * 1e-39).astype(np.float32)           # subnormal
        v[1::11] = rng.uniform(-1, 1, len(v[1::11])).astype(np.float32) * np.float32(2.0 ** -149 * 7)
        if huge_floats:
            v[2::13] = np.finfo(np.float32).max
            v[3::13] = -np.finfo(np.float32).max
    else:
        v = 1.0 + rng.integers(1, 2 ** 20, n) * 2.0 ** -40                                     # more than 24 bits
        v[::3] = rng.normal(0, 1e6, len(v[::3])) + 2.0 ** -30
        if huge_floats:
            v[1::9] = rng.uniform(-1e300, 1e300, len(v[1::9]))
        v[2::9] = 5e-324 * rng.integers(1, 100, len(v[2::9]))                                   # f64 subnormal
    return v.reshape(shape)
