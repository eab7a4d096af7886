"""The cubic B-spline link of include/frog_chain.h restated in NumPy f64, a plain Newton polish on it, and the inputs and
assertions that pin FROG_T_BSPLINE_INVERSE (bspline_inverse in frog_amd/csrc/device/chain.hip, and its restatement in
oracle/chain_oracle.cpp) for accuracy.  Nothing here calls the device or the C++ oracle: the check_* functions take the
evaluator under test as a callable, so tests/test_chain.py (oracle) and tests/test_gpu_inverse.py (device) assert the same.

    forward     u = (x - origin) / spacing clamped to [-3, dims + 1], cell floor(u), taps cell - 1 .. cell + 2 per axis, the
                basis F0..F3 of registration/imageGroup.cxx:221-232 and its derivative, a tap outside the lattice contributes
                zero;  y = x + d,  J = I + dd / spacing
    polish      undamped Newton on T(x) = p from a given x: the reference root an inverse is measured against

What the inverse may be held to.  It stops at a point x whose Newton step delta and residual are both below 1e-3, without
applying that step.  The root is at x - delta + O(|delta|^2 |T''| / |J|); on the lattices below the second-order term is
about 5e-8, so a converged x lies within 1.05e-3 of the root (5 % for that term and for the solver), two implementations
within 2.1e-3 of each other, and a chain of three such links and a matrix, whose determinant stays above 0.29, returns
within 3e-3.  A point that does not converge in 500 iterations comes back as the last point of decreasing residual: never
worse than the first guess p - d(p)."""
import functools

import numpy as np

from frog_amd.chain import BSPLINE, BSPLINE_INVERSE, LINEAR, Link

F8 = np.float64
TOLERANCE = 1e-3                    # INVERSE_TOLERANCE of chain.hip, vtkWarpTransform's default
ROOT_DISTANCE = 1.05e-3
PAIR_DISTANCE = 2.1e-3
ROUND_TRIP = 3e-3
STRONG_FRAC, FOLDED_FRAC, PYRAMID_FRAC = 0.6, 2.0, 0.4
N_POINTS = 20000


# ---- the link ---------------------------------------------------------------------------------------------------------------
def basis(f):
    """(F, G), each (N, 4): the uniform cubic B-spline weights at fraction f and their derivatives."""
    F3 = f * f * f / 6
    F0 = (f * f - f) / 2 - F3 + 1.0 / 6
    F2 = f + F0 - F3 * 2
    F1 = 1 - F0 - F2 - F3
    G = np.stack([-(1 - f) * (1 - f) / 2, 1.5 * f * f - 2 * f, -1.5 * f * f + f + 0.5, f * f / 2], -1)
    return np.stack([F0, F1, F2, F3], -1), G


def _taps(link, pts):
    """Per axis (first tap index (N,), weights F (N, 4), derivative weights G (N, 4), tap on the lattice (N, 4))."""
    out = []
    for k in range(3):
        raw = (pts[:, k] - F8(link.origin[k])) / F8(link.spacing[k])
        u = np.fmin(np.fmax(raw, -3.0), F8(link.dims[k] + 1))        # fmax/fmin drop a NaN, as the C functions do
        fl = np.floor(u)
        F, G = basis(u - fl)
        i0 = fl.astype(np.int64) - 1
        idx = i0[:, None] + np.arange(4)
        out.append((idx, F, G, (idx >= 0) & (idx < link.dims[k])))
    return out


def forward(link, pts):
    """(y, J) of a lattice link (forward, whatever its kind says) at pts (N, 3): y (N, 3), J = dy/dx (N, 3, 3)."""
    pts = np.ascontiguousarray(pts, F8).reshape(-1, 3)
    nx, ny, nz = link.dims
    c = link.coeffs.astype(F8).reshape(nz, ny, nx, 3)               # widened exactly; x fastest
    (ix, Fx, Gx, okx), (iy, Fy, Gy, oky), (iz, Fz, Gz, okz) = _taps(link, pts)
    Fx, Gx = np.where(okx, Fx, 0.0), np.where(okx, Gx, 0.0)
    Fy, Gy = np.where(oky, Fy, 0.0), np.where(oky, Gy, 0.0)
    Fz, Gz = np.where(okz, Fz, 0.0), np.where(okz, Gz, 0.0)
    ix, iy, iz = np.clip(ix, 0, nx - 1), np.clip(iy, 0, ny - 1), np.clip(iz, 0, nz - 1)
    taps = c[iz[:, :, None, None], iy[:, None, :, None], ix[:, None, None, :]]      # (N, 4z, 4y, 4x, 3)

    def blend(wz, wy, wx):
        w = wz[:, :, None, None] * wy[:, None, :, None] * wx[:, None, None, :]
        return (w[..., None] * taps).sum(axis=(1, 2, 3))

    y = pts + blend(Fz, Fy, Fx)
    J = np.zeros((len(pts), 3, 3), F8)
    for col, dd in enumerate((blend(Fz, Fy, Gx), blend(Fz, Gy, Fx), blend(Gz, Fy, Fx))):
        J[:, :, col] = dd / F8(link.spacing[col])
        J[:, col, col] += 1.0
    return y, J


def support(link, pts):
    """(none, partial): points none of whose 64 taps is on the lattice (u < -2 or u >= dims + 1 on some axis), and points
    with some taps on it and some off."""
    pts = np.ascontiguousarray(pts, F8).reshape(-1, 3)
    counts = np.stack([ok.sum(1) for _, _, _, ok in _taps(link, pts)], -1)
    none = (counts == 0).any(1)
    return none, ~none & (counts < 4).any(1)


def chain_forward(links, pts):
    """(y, J) of a chain of linear and forward lattice links: J the product of the links' Jacobians at the successive points."""
    p = np.ascontiguousarray(pts, F8).reshape(-1, 3)
    A = np.broadcast_to(np.eye(3), (len(p), 3, 3))
    for link in links:
        if link.kind == LINEAR:
            p, J = p @ link.matrix[:3, :3].T + link.matrix[:3, 3], np.broadcast_to(link.matrix[:3, :3], (len(p), 3, 3))
        elif link.kind == BSPLINE:
            p, J = forward(link, p)
        else:
            raise ValueError("the restatement covers linear and forward B-spline links")
        A = J @ A
    return p, A


def polish(link, x, p):
    """Plain Newton from x on T(x) = p, per point until its step is below 1e-12 or 20 iterations have run: (root, |T(root) - p|)."""
    x = np.array(x, F8).reshape(-1, 3)
    p = np.ascontiguousarray(p, F8).reshape(-1, 3)
    active = np.arange(len(x))
    with np.errstate(all="ignore"):
        for _ in range(20):
            if not len(active):
                break
            y, J = forward(link, x[active])
            step = np.linalg.solve(J, (y - p[active])[..., None])[..., 0]
            x[active] -= step
            active = active[~(np.linalg.norm(step, axis=1) < 1e-12)]
        return x, np.linalg.norm(forward(link, x)[0] - p, axis=1)


# ---- the inputs --------------------------------------------------------------------------------------------------------------
def _frozen(a):
    a.setflags(write=False)
    return a


def _lattice(rng, dims, origin, spacing, frac):
    co = frac * spacing * rng.uniform(-1.0, 1.0, (dims[0] * dims[1] * dims[2], 3))
    link = Link.bspline(dims, (origin,) * 3, (spacing,) * 3, co.astype(np.float32))
    _frozen(link.coeffs)
    return link


@functools.lru_cache(maxsize=None)
def strong_lattice(frac, seed=2):
    """One lattice of 11 x 11 x 12 control points 12 mm apart whose coefficients are frac * spacing * uniform(-1, 1): fold-free
    at frac 0.6 (smallest determinant about a third), folded at 2.0.  Covers [0, 96] x [0, 96] x [0, 108] with full support."""
    return _lattice(np.random.default_rng(seed), (11, 11, 12), -12.0, 12.0, frac)


MATRIX = np.array([[1.05, .08, 0, 4], [-.06, .95, .03, -3], [.02, 0, 1.1, 2], [0, 0, 0, 1.0]])


@functools.lru_cache(maxsize=None)
def pyramid_chain(frac=PYRAMID_FRAC, seed=1):
    """A matrix, then lattices of 4, 8 and 16 cells over 96 mm, as frog's pyramid refines them: fold-free at frac 0.4."""
    rng = np.random.default_rng(seed)
    links = [Link.linear(MATRIX)]
    for n in (4, 8, 16):
        links.append(_lattice(rng, (n + 3, n + 3, n + 4), -96.0 / n, 96.0 / n, frac))
    return tuple(links)


@functools.lru_cache(maxsize=None)
def sample_points(seed, n=N_POINTS):
    """n points of uniform(-40, 140)^3: inside the lattices, on their borders (partial support) and beyond them."""
    return _frozen(np.random.default_rng(seed).uniform(-40.0, 140.0, (n, 3)))


CHECK_GRID = ((0.0, 0.0, 0.0), (1.6, 1.6, 1.8), (60, 60, 60))      # the full-support box of strong_lattice, 60^3 nodes
JACOBIAN_GRID = ((2.0, 2.0, 2.0), (4.0, 4.0, 4.0), (24, 24, 24))   # the pyramid's interior


def inverse_link(link):
    return Link(BSPLINE_INVERSE, dims=link.dims, origin=link.origin, spacing=link.spacing, coeffs=link.coeffs)


def non_finite_points():
    """Twelve points with NaN, +inf or -inf in one coordinate each, the other two inside the lattices."""
    pts = np.random.default_rng(8).uniform(10.0, 80.0, (12, 3))
    for k, bad in enumerate([np.nan, np.inf, -np.inf] * 4):
        pts[k, k % 3 if k < 9 else (k + 1) % 3] = bad
    return pts


# ---- the assertions, for any evaluator apply(links, points) -> (N, 3) ---------------------------------------------------------
def _norm(v):
    return np.linalg.norm(v, axis=1)


def check_strong(apply, report=lambda name, value: None):
    """(a) the fold-free lattice: every point converges onto the unique root.  Returns the evaluator's x."""
    link, p = strong_lattice(STRONG_FRAC), sample_points(5)
    x = apply([inverse_link(link)], p)
    assert x.shape == p.shape and np.isfinite(x).all()
    none, partial = support(link, p)
    assert none.sum() >= 1000 and partial.sum() >= 1000, (none.sum(), partial.sum())
    assert np.array_equal(x[none], p[none])                         # no tap: d = 0, the first guess is p and its residual 0
    residual = _norm(forward(link, x)[0] - p)
    report("strong_max_residual", residual.max())
    assert residual.max() < TOLERANCE
    root, root_residual = polish(link, x, p)
    assert root_residual.max() < 1e-10                              # the reference itself converged
    distance = _norm(x - root)
    report("strong_max_distance_to_root", distance.max())
    assert distance.max() <= ROOT_DISTANCE
    return x


def check_stages(apply, inv):
    """(b) the inverted pyramid link by link: the chain is the composition of its links, no state carried from one Newton
    solve into the next, and every lattice stage solves its own equation.  Returns (p, x)."""
    p = sample_points(6, 4000)
    stage = [p]
    for link in inv:
        stage.append(apply([link], stage[-1]))
    x = apply(list(inv), p)
    assert np.array_equal(x, stage[-1])
    for k, link in enumerate(inv):
        if link.kind == BSPLINE_INVERSE:
            residual = _norm(forward(link, stage[k + 1])[0] - stage[k])
            assert residual.max() < TOLERANCE, (k, residual.max())
    return p, x


def check_round_trip(p, x, report=lambda name, value: None):
    back = _norm(chain_forward(pyramid_chain(), x)[0] - p)
    report("pyramid_max_round_trip", back.max())
    assert back.max() < ROUND_TRIP


def stage_jacobian(apply, inv, nodes):
    """The Jacobian of the forward chain along the inverse's own path: F = J_0(x_1) J_1(x_2) ..., link k of the inverted chain
    taking x_k to x_{k+1} and J_k the forward Jacobian of that link at its output x_{k+1}.  The inverse stops 1e-3 short of
    each root, so the forward chain started from the final x alone visits other points and its Jacobian differs by about
    1e-4; along the inverse's path (Jacobian of the inverse) F = I to rounding."""
    F = np.broadcast_to(np.eye(3), (len(nodes), 3, 3))
    q = nodes
    for link in inv:
        q = apply([link], q)
        if link.kind == BSPLINE_INVERSE:
            F = F @ forward(link, q)[1]
        else:
            F = F @ np.linalg.inv(link.matrix[:3, :3])
    return F


def stage_determinant(apply, inv, nodes):
    return np.linalg.det(stage_jacobian(apply, inv, nodes))


def check_folded(apply, report=lambda name, value: None):
    """(d) the folded lattice: termination and the fallback, not a root."""
    link, p = strong_lattice(FOLDED_FRAC), sample_points(5)
    x = apply([inverse_link(link)], p)
    assert np.isfinite(x).all()
    first = p - (forward(link, p)[0] - p)
    residual, first_residual = _norm(forward(link, x)[0] - p), _norm(forward(link, first)[0] - p)
    assert (residual <= first_residual * (1 + 1e-12)).all(), np.max(residual - first_residual)
    # Every point whose residual is below the tolerance is a root to within ROOT_DISTANCE, but for one kind: a point on the
    # fold itself.  det J changes by about |J|^2 |T''| ~ 1 per mm here, so |det J(x)| < 1e-3 puts the fold within about a
    # tolerance of x: the two preimages that merge there are not told apart at 1e-3, Newton's step is unbounded and no root
    # need be near.  On these bytes one point of 20 000 comes back from the fallback like that (residual 6.7e-5,
    # det J = -6.6e-8, the next smallest |det J| among the solved points is 0.057).  At most three may be set aside, and
    # they count as unsolved in the cap.
    det = np.abs(np.linalg.det(forward(link, x)[1]))
    on_fold = (residual < TOLERANCE) & (det < 1e-3)
    report("folded_points_on_the_fold", int(on_fold.sum()))
    assert on_fold.sum() <= 3
    solved = (residual < TOLERANCE) & ~on_fold
    share = 1.0 - solved.mean()
    report("folded_unsolved_share", share)
    root, root_residual = polish(link, x[solved], p[solved])
    assert root_residual.max() < 1e-10
    distance = _norm(x[solved] - root)
    report("folded_max_distance_to_root", distance.max())
    assert distance.max() <= ROOT_DISTANCE
    assert share <= 0.05
    return x
