"""A group of images whose points sit where the lattice kernels switch paths, and an f64 restatement of one deformable
step and of the B-spline transform to compare them with, node by node (tests/test_lattice_design.py on the CPU oracle,
tests/test_gpu_lattice_design.py on the device).

The frame.  Every image begins with the points (0,0,0) and (64,64,64) and every other point lies in [0,64]^3: all images
have the same bounding box, the linear initialisation is the identity, and with initial_grid_size 8, bounding_box_margin 0.25
the lattices are exact in f64 (LATTICES below): level 0 has spacing 8 and origin -24, so a coordinate 8 m has the lattice
coordinate m + 3 and the fraction 0 -- to the bit.

The links.  Images 1 and 2 are copies of image 0 moved by at most 0.02 per axis; point k is linked to point k in the blocks
(0,1), (0,2), (1,2).  Every link is shorter than 0.1 mm, so its weight is exactly 1 (stats.h:87), every linked point has
sWeight exactly 2 and the sweep plays no part in what the lattice kernels are handed.  Image 3 is the frame alone, image 4
the frame and (32,32,32): neither has a link.

The restatement is numpy f64 and shares no code with the oracle or with lattice_util.lattice_taps; it is handed the run's own
per-point sums, coordinates and previous coefficients, so that only the scatter and the control-point step are compared.
The bound on a coefficient is derived (see `step`), it is not measured.
"""
import numpy as np

OPTIONS = dict(initial_grid_size=8.0, bounding_box_margin=0.25, guarantee_diffeomorphism=0)
# level: (cells per axis, spacing, origin, control points per axis)
LATTICES = {0: (12, 8.0, -24.0, 15), 1: (24, 4.0, -20.0, 27), 2: (48, 2.0, -18.0, 51), 3: (96, 1.0, -17.0, 99)}
N_IMAGES = 5
SCATTER_CHUNK = 384                  # k_grid.hip.h: points per scatter block
FULL_BRICKS = {(0, 0, 0): 384, (2, 0, 0): 385, (0, 2, 0): 768}      # level-0 bricks of 4^3 cells (bx, by, bz): points of image 0
CROWDED_CELL = (24.0, 32.0)          # the level-0 cell [24, 32)^3 holds 1000 points more
LONE = np.array([48.0 + 2.0 ** -11, 48.0 + 2.0 ** -11, 48.0 + 2.0 ** -12])      # fractions 2^-14, 2^-14, 2^-15 at level 0
RESERVED = 39.9                      # no other linked point has all three coordinates above this: LONE's far nodes are its own
FLUSH = 2.0 ** -150                  # a term below this vanishes in any f32 accumulator
U = 2.0 ** -24                       # unit round-off of f32
TINY = 2.0 ** -149                   # smallest f32 denormal
ALL_IMAGES = "all images"            # step(mean_over=...): the mean of the proposals over every image of the group


class Lattice:
    """dims, origin, spacing of a lattice (from a frog_grid_info or from LATTICES)."""

    def __init__(self, dims, origin, spacing):
        self.dims = np.array([int(d) for d in dims], np.int64)
        self.origin = np.array([float(o) for o in origin], np.float64)
        self.spacing = np.array([float(s) for s in spacing], np.float64)
        self.n_cp = int(np.prod(self.dims))

    @classmethod
    def of(cls, info):
        return cls(list(info.dims), list(info.origin), list(info.spacing))

    @classmethod
    def level(cls, level):
        cells, spacing, origin, dims = LATTICES[level]
        return cls([dims] * 3, [origin] * 3, [spacing] * 3)


# ---- the points ----------------------------------------------------------------------------------------------------------

def _image0(rng):
    f32 = np.float32
    parts = []
    m8 = 8.0 * np.arange(9)
    # on faces: multiples of 8 on three, two and one axes (0, 64 and the multiples of 16 and 32 -- brick faces -- among them)
    parts.append(np.stack(np.meshgrid(m8, m8, m8, indexing="ij"), axis=-1).reshape(-1, 3))
    for free in range(3):
        for n in (100, 100):
            p = rng.choice(m8, size=(n, 3))
            p[:, free] = rng.uniform(0, 64, n)
            parts.append(p)
        p = rng.uniform(0, 64, (100, 3))
        p[:, free] = rng.choice(m8, size=100)
        parts.append(p)
    # one ulp off a face: nextafter of 8 m toward each side, m = 1..7, on one axis and on all three
    below = np.nextafter((8.0 * np.arange(1, 8)).astype(f32), f32(0)).astype(np.float64)
    above = np.nextafter((8.0 * np.arange(1, 8)).astype(f32), f32(100)).astype(np.float64)
    for axis in range(3):
        for side in (below, above):
            p = rng.uniform(0, 64, (7 * 12, 3))
            p[:, axis] = np.repeat(side, 12)
            parts.append(p)
    parts.append(np.stack(np.meshgrid(below, below, below, indexing="ij"), axis=-1).reshape(-1, 3))
    mixed = np.stack(np.meshgrid(np.arange(7), np.arange(7), np.arange(7), indexing="ij"), axis=-1).reshape(-1, 3)
    pick = rng.integers(0, 2, mixed.shape).astype(bool)
    parts.append(np.where(pick, below[mixed], above[mixed]))
    # tails: level-0 fractions 2^-17 .. 2^-13 on two axes (the third anywhere) and on three
    ks = np.arange(13, 18)
    for free in range(3):
        a, b = np.meshgrid(ks, ks, indexing="ij")
        p = np.empty((25, 3))
        cell = 8.0 * rng.integers(1, 5, (25, 3))
        p[:, (free + 1) % 3] = cell[:, 0] + 8.0 * 2.0 ** -a.ravel()
        p[:, (free + 2) % 3] = cell[:, 1] + 8.0 * 2.0 ** -b.ravel()
        p[:, free] = rng.uniform(0, 64, 25)
        parts.append(p)
    a, b, c = np.meshgrid(ks, ks, ks, indexing="ij")
    cell = 8.0 * rng.integers(1, 5, (125, 3))
    parts.append(cell + 8.0 * 2.0 ** -np.stack([a.ravel(), b.ravel(), c.ravel()], axis=-1).astype(np.float64))
    # a cell with more points than a scatter block holds
    parts.append(rng.uniform(CROWDED_CELL[0] + 0.01, CROWDED_CELL[1] - 0.01, (1000, 3)))
    # generic
    parts.append(rng.uniform(0, 64, (1500, 3)))
    pts = np.concatenate(parts).astype(f32)
    assert np.all(pts >= 0) and np.all(pts <= 64)
    pts = pts[~np.all(pts > RESERVED, axis=1)]              # the reserved corner stays empty ...
    pts = np.concatenate([pts, LONE[None].astype(f32)])     # ... but for the lone tail point
    # bricks of exactly 384, 385 and 768 points: top up with points inside the brick
    frame = np.array([[0, 0, 0], [64, 64, 64]], f32)
    lat = Lattice.level(0)
    for brick, want in FULL_BRICKS.items():
        have = int(np.count_nonzero(np.all(brick_of(np.concatenate([frame, pts]), lat, 4) == np.array(brick), axis=1)))
        assert have < want, (brick, have)
        lo = np.array([0.0 if b == 0 else 16.0 if b == 1 else 48.0 for b in brick])
        hi = np.array([16.0 if b == 0 else 48.0 if b == 1 else 64.0 for b in brick])
        pts = np.concatenate([pts, rng.uniform(lo + 0.05, hi - 0.05, (want - have, 3)).astype(f32)])
    return np.concatenate([frame, pts])


def build(seed=20):
    """(point_offset, xyz f32 [n, 3], blocks) of the designed group."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    img0 = _image0(rng)
    n = len(img0)
    frame = img0[:2]
    images = [img0]
    for sign in (1.0, -1.0):
        # a common shift, so that a control point's mean over its points does not average the displacement away
        shift = sign * 0.0115 * np.array([1.0, -1.0, 1.0]) + rng.uniform(-0.008, 0.008, (n, 3))
        moved = np.clip((img0.astype(np.float64) + shift).astype(f32), f32(0), f32(64))
        moved[:2] = frame
        images.append(moved)
    images.append(frame.copy())
    images.append(np.concatenate([frame, np.array([[32, 32, 32]], f32)]))
    po = np.concatenate([[0], np.cumsum([len(a) for a in images])])
    k = np.arange(2, n, dtype=np.uint32)                    # the frame has no links
    blocks = [(0, 1, k, k), (0, 2, k, k), (1, 2, k, k)]
    return po, np.concatenate(images), blocks


_pairs = {}


def pairs(seed=20):
    """The group as frog_amd.pairs.Pairs (built once)."""
    from frog_amd.pairs import Pairs
    if seed not in _pairs:
        _pairs[seed] = Pairs.from_arrays(*build(seed))
    return _pairs[seed]


# ---- where the scatter and the sort put a point --------------------------------------------------------------------------

def cells32(x, lat):
    """Cell and fraction as imageGroup.cxx:303-310 computes them: the f64 quotient rounded to f32, then floor."""
    q = ((np.asarray(x, np.float32).astype(np.float64) - lat.origin) / lat.spacing).astype(np.float32)
    c = np.floor(q)
    return c.astype(np.int64), (q - c).astype(np.float64)


def cells64(x, lat):
    """Cell and fraction as vtkBSplineTransform computes them: f64 throughout."""
    q = (np.asarray(x, np.float32).astype(np.float64) - lat.origin) / lat.spacing
    c = np.floor(q)
    return c.astype(np.int64), q - c


def brick_of(x, lat, brick):
    """Brick (bx, by, bz) a point is sorted into: point_key's rule (k_grid.hip.h)."""
    c = np.maximum(cells32(x, lat)[0] - 1, 0)
    nb = (lat.dims - 3 + brick - 1) // brick
    return np.minimum(c // brick, nb - 1)


def outside(x, lat):
    """Points whose 0-based cell lies outside [0, cells) on some axis: part of their stencil is outside the lattice."""
    c = cells32(x, lat)[0] - 1
    return np.any((c < 0) | (c >= lat.dims - 3), axis=1)


def stray(x, lat, brick):
    """Points whose stencil is not inside the tile of the brick point_key clamps them into: the ones the scatter sends through
    its stray path and frog_test_stray_points counts.  The bricks cover ceil(cells / brick) * brick cells per axis, so a point
    beyond the lattice's last cell but inside the last brick is `outside` and no stray: its taps outside the lattice stay in
    the tile, where the lattice step never looks."""
    c = cells32(x, lat)[0] - 1
    nb = (lat.dims - 3 + brick - 1) // brick
    local = c - np.minimum(np.maximum(c, 0) // brick, nb - 1) * brick
    return np.any((local < 0) | (local >= brick), axis=1)


def classes(x, lat, brick=4):
    """Counts of the designed classes among the points x of one image on lattice `lat`."""
    c32, f32 = cells32(x, lat)
    c64, _ = cells64(x, lat)
    differs = c32 != c64
    at_brick_face = differs & ((c32 - 1) % brick == 0) & (c32 - 1 > 0)      # sorted above a brick face, evaluated below it
    out = {"fraction_zero": [int(v) for v in np.count_nonzero(f32 == 0, axis=0)],
           "cell_differs": [int(v) for v in np.count_nonzero(differs, axis=0)],
           "brick_face": int(np.count_nonzero(np.any(at_brick_face, axis=1)))}
    tail = (f32 > 0) & (f32 <= 2.0 ** -13) & (f32 >= 2.0 ** -17)
    out["tails_two_axes"] = int(np.count_nonzero(tail.sum(axis=1) == 2))
    out["tails_three_axes"] = int(np.count_nonzero(tail.sum(axis=1) == 3))
    # tail points on three axes alone in their 3 x 3 x 3 block of cells
    lone = 0
    for p in np.nonzero(tail.sum(axis=1) == 3)[0]:
        near = np.all(np.abs(c32 - c32[p]) <= 1, axis=1)
        lone += int(np.count_nonzero(near) == 1)
    out["lone_tails"] = lone
    _, per_cell = np.unique(c32, axis=0, return_counts=True)
    out["largest_cell"] = int(per_cell.max())
    b = brick_of(x, lat, brick)
    out["bricks"] = {k: int(np.count_nonzero(np.all(b == np.array(k), axis=1))) for k in FULL_BRICKS}
    return out


# ---- the restatement -----------------------------------------------------------------------------------------------------

def cubic(f):
    """imageGroup.cxx:221-232 in f64; f [n] -> [n, 4]."""
    f2 = f * f
    w3 = f2 * f * (1.0 / 6.0)
    w0 = (f2 - f) * 0.5 - w3 + 1.0 / 6.0
    w2 = f + w0 - w3 * 2
    w1 = 1 - w0 - w2 - w3
    return np.stack([w0, w1, w2, w3], axis=-1)


def _stencil(cell, frac, lat):
    """Nodes [n, 64] (-1: outside the lattice) and weights (wx wy) wz [n, 64], tap i + 4 j + 16 k."""
    wx, wy, wz = cubic(frac[:, 0]), cubic(frac[:, 1]), cubic(frac[:, 2])
    o = np.arange(4)
    gx = cell[:, 0, None] - 1 + o; gy = cell[:, 1, None] - 1 + o; gz = cell[:, 2, None] - 1 + o
    ok = lambda g, d: (g >= 0) & (g < d)
    inside = (ok(gz, lat.dims[2])[:, :, None, None] & ok(gy, lat.dims[1])[:, None, :, None] & ok(gx, lat.dims[0])[:, None, None, :])
    node = gx[:, None, None, :] + lat.dims[0] * (gy[:, None, :, None] + lat.dims[1] * gz[:, :, None, None])
    w = (wx[:, None, None, :] * wy[:, None, :, None]) * wz[:, :, None, None]
    n = len(cell)
    return np.where(inside, node, -1).reshape(n, 64), w.reshape(n, 64)


def step(lat, point_offset, xyz, sums, c_prev, alpha, touched_only=False, mean_over=ALL_IMAGES, first_image=0):
    """One deformable step of all images in f64 (imageGroup.cxx:299-432).

    xyz [P, 3]: the coordinates the scatter bins (Point::xyz); sums [P, 4]: per-point (sDisp, sWeight); c_prev: per image
    the coefficients before the step, [n_cp, 3].  Returns a dict:
      nodes   the control points the arrays below are about (all of them, or with touched_only those some image's gradient
              reaches: at every other node the proposal is the previous coefficient)
      new     [images, nodes, 3] proposal minus the mean of the proposals over the images
      bound   [images, nodes, 3] what |new - computed| may be for ANY order of f32 additions of terms that carry six roundings
              each (three weights, two products, the multiply-add): with n the terms reaching a node,
                B = (n + 6) 2^-24 sum |w s| + n 2^-149                        bounds the error of a gradient sum,
                D = alpha (B_g + |g / gw| B_gw) / gw + 2 2^-24 |proposal|     the proposal's (first order; 0 where gw == 0),
                D_i + mean_j D_j + 2^-24 (|proposal| + |mean|) + 2^-149       the coefficient's
      gw      [images, nodes] the weight sums;  terms [images, nodes] the n above

    mean_over: the divisor of the sum of the proposals (ALL_IMAGES: the number of images, a context that owns the whole group; an
    int: the group's image count, whatever part of the group the sum runs over), or None: no mean is removed, the form with
    fixed images (imageGroup.cxx:398).  The coefficient is then the proposal itself -- (float)((double) v - 0.0) is v --, and
    the terms the mean brings drop out of the bound:
                D_i + 2^-24 |proposal| + 2^-149                                the coefficient's without a mean
    first_image: the images below it take no part (the fixed images: every loop of the step starts behind them): they add nothing
    to the sum, their rows of `new` are their previous coefficients, of `bound` 2^-149, of `gw` and `terms` zero.
    """
    n_img = len(point_offset) - 1
    per = []
    touched = []
    for i in range(first_image, n_img):
        x = np.asarray(xyz[point_offset[i]:point_offset[i + 1]], np.float32)
        s = np.asarray(sums[point_offset[i]:point_offset[i + 1]], np.float32).astype(np.float64)
        live = s[:, 3] != 0                                 # imageGroup.cxx:299
        cell, frac = cells32(x[live], lat)
        node, w = _stencil(cell, frac, lat)
        t = w[:, :, None] * s[live][:, None, :]             # [n, 64, 4]
        t[np.abs(t) < FLUSH] = 0.0
        keep = (node >= 0) & np.any(t != 0, axis=2)
        node, t = node[keep], t[keep]                       # [m], [m, 4]
        un, inv = np.unique(node, return_inverse=True)
        g = np.stack([np.bincount(inv, weights=t[:, k], minlength=len(un)) for k in range(4)], axis=-1)
        a = np.stack([np.bincount(inv, weights=np.abs(t[:, k]), minlength=len(un)) for k in range(4)], axis=-1)
        n = np.bincount(inv, minlength=len(un)).astype(np.float64)
        per.append((un, g, a, n))
        touched.append(un)
    nodes = np.unique(np.concatenate(touched)) if touched_only else np.arange(lat.n_cp)
    m = len(nodes)
    prop = np.empty((n_img, m, 3)); D = np.zeros((n_img, m, 3)); gw_all = np.zeros((n_img, m)); terms = np.zeros((n_img, m))
    for i in range(first_image):
        prop[i] = np.asarray(c_prev[i], np.float32).astype(np.float64)[nodes]
    for i, (un, g, a, n) in enumerate(per, start=first_image):
        at = np.searchsorted(nodes, un)
        G = np.zeros((m, 4)); A = np.zeros((m, 4)); N = np.zeros(m)
        G[at], A[at], N[at] = g, a, n
        B = (N[:, None] + 6) * U * A + N[:, None] * TINY
        c = np.asarray(c_prev[i], np.float32).astype(np.float64)[nodes]
        gw = G[:, 3]
        move = gw > 0
        ratio = np.zeros((m, 3))
        ratio[move] = G[move, :3] / gw[move, None]
        prop[i] = c + alpha * ratio
        D[i][move] = alpha * (B[move, :3] + np.abs(ratio[move]) * B[move, 3:4]) / gw[move, None] + 2 * U * np.abs(prop[i][move])
        gw_all[i], terms[i] = gw, N
    if mean_over is None:
        new = prop.copy()
        bound = D + U * np.abs(prop) + TINY
    else:
        divisor = n_img if mean_over is ALL_IMAGES else int(mean_over)
        mean = prop[first_image:].sum(axis=0) / divisor         # (all images: prop.mean(axis=0), the same two operations)
        new = prop - mean
        bound = D + D[first_image:].sum(axis=0) / divisor + U * (np.abs(prop) + np.abs(mean)) + TINY
    new[:first_image] = prop[:first_image]
    bound[:first_image] = TINY
    return {"nodes": nodes, "new": new, "bound": bound, "gw": gw_all, "terms": terms}


def transform(lat, x, c):
    """vtkBSplineTransform, BorderModeZero, in f64: (float)(x + sum w c), taps outside the lattice dropped; separable
    accumulation x -> y -> z.  x [n, 3] f32, c [n_cp, 3] f32 of the points' image.  Returns (f32 [n, 3], f64 displacement)."""
    x = np.asarray(x, np.float32)
    c = np.asarray(c, np.float32).astype(np.float64)
    cell, frac = cells64(x, lat)
    F = [cubic(frac[:, k]) for k in range(3)]
    i0 = cell - 1
    n = len(x)
    disp = np.zeros((n, 3))
    for k in range(4):
        z = i0[:, 2] + k
        okz = (z >= 0) & (z < lat.dims[2])
        vz = np.zeros((n, 3))
        for j in range(4):
            y = i0[:, 1] + j
            oky = okz & (y >= 0) & (y < lat.dims[1])
            vy = np.zeros((n, 3))
            for i in range(4):
                xx = i0[:, 0] + i
                ok = oky & (xx >= 0) & (xx < lat.dims[0])
                node = np.where(ok, xx + lat.dims[0] * (y + lat.dims[1] * z), 0)
                vy += np.where(ok[:, None], c[node] * F[0][:, i, None], 0.0)
            vz += np.where(oky[:, None], vy * F[1][:, j, None], 0.0)
        disp += np.where(okz[:, None], vz * F[2][:, k, None], 0.0)
    return (x.astype(np.float64) + disp).astype(np.float32), disp


def energy(point_offset, blocks, xyz2):
    """sqrt(sum w^2 d^2 / sum w^2) over the half-links with every weight 1, in f64."""
    x = np.asarray(xyz2, np.float32).astype(np.float64)
    d2 = []
    for i, j, p, q in blocks:
        d = x[point_offset[i] + p.astype(np.int64)] - x[point_offset[j] + q.astype(np.int64)]
        d2.append(np.sum(d * d, axis=1))
    d2 = np.concatenate(d2)
    return float(np.sqrt(d2.sum() / len(d2))), float(np.sqrt(d2.max()))


def worst_ratio(new, bound, got):
    """Largest |got - new| / bound, and where: (ratio, image, index into nodes, component)."""
    r = np.abs(np.asarray(got, np.float64) - new) / bound
    at = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[at]), at


def node_class(x, lat, node, gw):
    """For the record of where the largest err / bound sits: which designed class the points x of the image that reach
    control point `node` (weight sum gw there) belong to -- 'stray', 'tail', 'crowded cell', 'face' or 'generic'."""
    cell, frac = cells32(x, lat)
    n3 = np.array([node % lat.dims[0], (node // lat.dims[0]) % lat.dims[1], node // (lat.dims[0] * lat.dims[1])])
    reach = np.all((n3 >= cell - 1) & (n3 <= cell + 2), axis=1)
    if np.any(outside(x, lat) & reach):
        return "stray"
    if 0 < gw < 2.0 ** -40:
        return "tail"
    if np.count_nonzero(reach) >= 600:
        return "crowded cell"
    if reach.any() and np.mean(np.any(frac[reach] == 0, axis=1)) > 0.3:
        return "face"
    return "generic"
