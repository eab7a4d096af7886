"""The coverage-aware Gaussian (frog_smooth_taps, frog_smooth_volume and frog_glm_smooth, include/frog_chain.h) restated in
NumPy, line by line: the taps by one rounded f64 operation per line, the two f64 fields num and den, three passes of
    acc = +0.0;  for d = -R .. +R ascending:  m = w_|d| * in(v + d * e_axis);  acc = acc + m
on whole arrays (one * and one + per step, a neighbour outside the grid entering as +0.0), and the one division.
`literal` is a second, independent form: voxel by voxel in Python floats over the participating neighbours inside the grid
alone, which is the same sum because no sum is ever -0.0 and so a term of +0.0 changes no bit."""
import numpy as np

F4, F8, U4 = np.float32, np.float64, np.uint32
NAN = U4(0x7FC00000).view(F4)
MAX_RADIUS = 64
FWHM = 2.3548200450309493


def radius(sigma, spacing):
    q = F8(3.0) * F8(sigma)
    q = q / F8(spacing)
    return int(np.ceil(q))


def taps(sigma, spacing, exp=np.exp):
    """(R, w_0 .. w_R) with `exp` for the exponential: the library's own taps are data, the tests take them from it."""
    R = radius(sigma, spacing)
    den = F8(2.0) * F8(sigma)
    den = den * F8(sigma)
    x = np.arange(R + 1).astype(F8) * F8(spacing)
    x = x * x
    x = x / den
    return R, exp(-x)


def taking(x, take=None):
    """Which voxels take part: a finite value and, with flags, a non-zero flag."""
    on = np.isfinite(np.asarray(x, F4))
    return on if take is None else on & (np.asarray(take) != 0)


def one_pass(field, w, axis):
    """One pass along `axis` of an f64 array: d ascending, one multiplication and one addition per step on the whole array."""
    R = len(w) - 1
    pad = [(0, 0)] * field.ndim
    pad[axis] = (R, R)
    padded = np.pad(field, pad)                                  # +0.0 outside the grid
    n = field.shape[axis]
    acc = np.zeros(field.shape, F8)
    for d in range(-R, R + 1):
        sl = [slice(None)] * field.ndim
        sl[axis] = slice(R + d, R + d + n)
        m = F8(w[abs(d)]) * padded[tuple(sl)]
        acc = acc + m
    return acc


def smooth(x, on, w3, fields=False):
    """x[z, y, x] float32, on bool, w3 = (taps along x, along y, along z): the smoothed float32 array, 0x7FC00000 where the
    voxel does not take part.  With `fields` also the two f64 fields after the three passes: (smoothed, num, den)."""
    x = np.asarray(x, F4)
    on = np.asarray(on, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        num = np.where(on, x.astype(F8), F8(0.0))
    den = np.where(on, F8(1.0), F8(0.0))
    for axis, w in ((2, w3[0]), (1, w3[1]), (0, w3[2])):
        num, den = one_pass(num, w, axis), one_pass(den, w, axis)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = (num / den).astype(F4)
    out = np.where(on, q, NAN)
    return (out, num, den) if fields else out


def literal(x, on, w3):
    """The same, voxel by voxel in Python floats (f64): the x pass over the participating neighbours alone, straight from
    the values, the y and z passes over the neighbours inside the grid alone."""
    x = np.asarray(x, F4)
    nz, ny, nx = x.shape
    on = np.asarray(on, bool)
    num = [[[float(x[z, y, i]) if on[z, y, i] else None for i in range(nx)] for y in range(ny)] for z in range(nz)]
    den = [[[1.0 if on[z, y, i] else None for i in range(nx)] for y in range(ny)] for z in range(nz)]

    def run(f, w, axis):
        R = len(w) - 1
        n = (nz, ny, nx)[axis]
        out = [[[0.0] * nx for _ in range(ny)] for _ in range(nz)]
        for z in range(nz):
            for y in range(ny):
                for i in range(nx):
                    at = [z, y, i]
                    c = at[axis]
                    acc = 0.0
                    for d in range(max(-R, -c), min(R, n - 1 - c) + 1):
                        at[axis] = c + d
                        if f[at[0]][at[1]][at[2]] is None:      # does not take part: no term
                            continue
                        m = float(w[abs(d)]) * f[at[0]][at[1]][at[2]]
                        acc = acc + m
                    out[z][y][i] = acc
        return out

    for axis, w in ((2, w3[0]), (1, w3[1]), (0, w3[2])):
        num, den = run(num, w, axis), run(den, w, axis)
    out = np.full(x.shape, NAN, F4)
    for z in range(nz):
        for y in range(ny):
            for i in range(nx):
                if on[z, y, i]:
                    out[z, y, i] = F4(num[z][y][i] / den[z][y][i])
    return out


def smooth_planes(planes, w3):
    """Stored planes (n,) + shape of a whole grid, 0x7FC00000 where an entry does not take part: each smoothed."""
    planes = np.asarray(planes, F4)
    return np.stack([smooth(p, p.view(U4) != U4(0x7FC00000), w3) for p in planes])
