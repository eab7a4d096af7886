"""A group of MANY small images for the control-point step (lattice_step_kernel / cp_center_kernel, k_grid.hip.h): the image
count is the parameter, so that a test can sit on the switches the kernel takes on it -- passes of 64 images, the 512 images
up to which proposals wait in registers, batches of 10 in cp_center_kernel -- and the number of images whose points reach a
node varies over the lattice, so that the sparse form's shared values and its count of them are exercised
(tests/test_step_design.py on the CPU oracle, tests/test_gpu_step_design.py on the device).  The restatement and its derived
bound are lattice_design.step's; this module holds the group, the oversize count and what the tests ask of the group.

The frame is lattice_design's: every image begins with (0,0,0) and (64,64,64), everything else lies in [0,64]^3, OPTIONS make
the linear stage the identity and level 0 the lattice of spacing 8, origin -24, 15 nodes per axis.

The images.  A base set of BASE points in [4,44]^3; image i >= 1 carries a copy moved by at most 0.02 per axis (a common shift
whose sign alternates with i, so that a node's mean does not average the displacement away):
  shared     a cluster of 12 points inside the cell [24,32)^3, 12 points spread over [8,32]^3 and one on three cell faces:
             every image has them; point k of image i is linked to point k of image i + 1, block (i, i + 1);
  thirds     6 points in [36,44] x [4,12] x [4,12] that only the images with i % 3 == 0 carry.  No neighbour has them, so
             the copy of image i is linked to the copy of image i + 3, block (i, i + 3);
  last two   6 points in [4,12] x [36,44] x [4,12] that only the images i >= n - 2 carry, linked in block (n - 2, n - 1).
Every link is shorter than 0.1 mm: its weight is exactly 1 (stats.h:87), a point's weight sum is the number of its links.
Nothing but the frame's far corner lies beyond 48 on two axes: large regions that no image reaches.

Image 0 also fills three "arms" -- [48,64] x [0,16)^2 and its two rotations -- with 4 * 384 + 1, 5 * 384 + 1 and 385 points,
partners in image 1.  A brick's points are cut into scatter blocks of SCATTER_CHUNK = 384 (brick_chunks_kernel: ceil(points /
384) slots), and lattice_step_kernel reads the slots behind the first four at a time: 5 slots are exactly one full trip of that
loop, 6 a second trip with one live entry and three clamped, 2 one trip with one live entry.  The set-up takes bricks of 4^3
cells or of 8^3 by the points per brick (make_geometry), which changes with the image count; an arm is a whole brick for
either edge on the 15^3 lattice (nothing else lies beyond 48 on one axis and below 48 on the others) and for the edge 4 on the
lattice of spacing 16, where the edge 8 makes one brick of each image: 11 slots for image 0.
"""
import numpy as np

import lattice_design as ld

OPTIONS = dict(ld.OPTIONS)
SCATTER_CHUNK = ld.SCATTER_CHUNK
N_SHARED, N_THIRDS, N_LAST = 25, 6, 6
BASE = N_SHARED + N_THIRDS + N_LAST
# image 0's arms: (axis beyond 48) -> points.  5, 6 and 2 scatter blocks
ARMS = {0: 4 * SCATTER_CHUNK + 1, 1: 5 * SCATTER_CHUNK + 1, 2: SCATTER_CHUNK + 1}
ARM_SLOTS = {0: 5, 1: 6, 2: 2}
# Two steps at alpha = 1 move some point by at least this much (2^8 ulps of 64): the second step starts from coefficients far
# from zero.  Two images stand 0.0115 apart per axis and meet half-way, less what the spline smooths away
MOVED = 2.0 ** 8 * 2.0 ** -17
# the lattices the tests run: name -> (options on top of OPTIONS, box handed to deformable_setup_bounds or None, dims, origin, spacing)
LATTICES = {
    # level 0 of the designed frame: 3375 nodes, the wide block shape (16 nodes), 3375 % 16 = 15: a partial last block
    "wide": ({}, None, [15, 15, 15], [-24.0] * 3, [8.0] * 3),
    # 729 nodes < LS_SMALL_NODES: the narrow block shape (4 nodes), 729 % 4 = 1: a partial last block
    "narrow": ({"initial_grid_size": 16.0}, None, [9, 9, 9], [-32.0] * 3, [16.0] * 3),
}
# exactly LS_SMALL_NODES = 2048 nodes (8 x 16 x 16), the first lattice that takes the wide shape: a box wider than the points on
# y and z.  Its spacing is no power of two; origin and spacing are read from the set-up's info
THRESHOLD = ({"initial_grid_size": 19.2}, ([0.0, -51.0, -51.0], [64.0, 115.0, 115.0]), [8, 16, 16])


def carries(i, n_images):
    """(thirds, last two, arms) of image i."""
    return i % 3 == 0, i >= n_images - 2, i < 2


def layout(i, n_images):
    """First index of each part in image i (None: the image does not carry it), and the image's point count."""
    thirds, last, arms = carries(i, n_images)
    at, out = 2 + N_SHARED, {"shared": 2}
    for name, has, n in (("thirds", thirds, N_THIRDS), ("last", last, N_LAST), ("arms", arms, sum(ARMS.values()))):
        out[name] = at if has else None
        at += n if has else 0
    return out, at


def _base(rng):
    cluster = rng.uniform(24.5, 31.5, (12, 3))
    spread = rng.uniform(8.0, 32.0, (12, 3))
    face = np.array([[16.0, 24.0, 16.0]])
    thirds = rng.uniform([36.0, 4.0, 4.0], [44.0, 12.0, 12.0], (N_THIRDS, 3))
    last = rng.uniform([4.0, 36.0, 4.0], [12.0, 44.0, 12.0], (N_LAST, 3))
    return np.concatenate([cluster, spread, face]), thirds, last


def _arms(rng):
    parts = []
    for axis, n in ARMS.items():
        lo, hi = np.full(3, 0.05), np.full(3, 15.95)
        lo[axis], hi[axis] = 48.05, 63.95
        parts.append(rng.uniform(lo, hi, (n, 3)))
    return np.concatenate(parts)


def build(n_images, seed=20):
    """(point_offset, xyz f32 [n, 3], blocks) of the group of n_images images.  Image i is the same for every n_images but for
    the parts it carries."""
    assert n_images >= 2
    f32 = np.float32
    rng = np.random.default_rng(seed)
    shared, thirds, last = _base(rng)
    arms = _arms(rng)
    frame = np.array([[0, 0, 0], [64, 64, 64]], f32)
    images = []
    for i in range(n_images):
        has_thirds, has_last, has_arms = carries(i, n_images)
        pts = np.concatenate([shared] + ([thirds] if has_thirds else []) + ([last] if has_last else []) + ([arms] if has_arms else []))
        if i:
            r = np.random.default_rng([seed, i])
            sign = 1.0 if i % 2 else -1.0
            # by part, so that a point's shift does not depend on which parts the image carries
            shift = {k: sign * 0.0115 * np.array([1.0, -1.0, 1.0]) + r.uniform(-0.008, 0.008, (n, 3))
                     for k, n in (("shared", N_SHARED), ("thirds", N_THIRDS), ("last", N_LAST), ("arms", len(arms)))}
            pts = pts + np.concatenate([shift["shared"]] + ([shift["thirds"]] if has_thirds else []) + ([shift["last"]] if has_last else [])
                                       + ([shift["arms"]] if has_arms else []))
        images.append(np.concatenate([frame, pts.astype(f32)]))
        assert len(images[-1]) == layout(i, n_images)[1] and images[-1].min() >= 0 and images[-1].max() <= 64
    po = np.concatenate([[0], np.cumsum([len(a) for a in images])])
    blocks = []
    for i in range(n_images):                                   # blocks in (image1, image2) order
        a, _ = layout(i, n_images)
        if i + 1 < n_images:
            b, _ = layout(i + 1, n_images)
            p, q = [a["shared"] + np.arange(N_SHARED)], [b["shared"] + np.arange(N_SHARED)]
            for name, n in (("last", N_LAST), ("arms", len(arms))):
                if a[name] is not None and b[name] is not None:
                    p.append(a[name] + np.arange(n)); q.append(b[name] + np.arange(n))
            blocks.append((i, i + 1, np.concatenate(p).astype(np.uint32), np.concatenate(q).astype(np.uint32)))
        if i % 3 == 0 and i + 3 < n_images:
            b, _ = layout(i + 3, n_images)
            k = np.arange(N_THIRDS)
            blocks.append((i, i + 3, (a["thirds"] + k).astype(np.uint32), (b["thirds"] + k).astype(np.uint32)))
    return po, np.concatenate(images), blocks


_pairs = {}


def pairs(n_images, seed=20):
    """The group as frog_amd.pairs.Pairs (built once per size)."""
    from frog_amd.pairs import Pairs
    if (n_images, seed) not in _pairs:
        _pairs[(n_images, seed)] = Pairs.from_arrays(*build(n_images, seed))
    return _pairs[(n_images, seed)]


# ---- what the tests ask of the group -------------------------------------------------------------------------------------

# The linear initialisation moves every image's anchor (32, 32, 32) onto the images' average, which it forms in f32 as the sum
# of n terms 32 / (float) n (imageGroup.cxx:823-824): exactly 32 for the image counts below -- there the frame is the model's to
# the bit and the lattices are LATTICES' --, within 2^-12 of it for the others (measured on the oracle: at most 1.9e-4, 577
# images), where the lattice's origin follows.  The restatement is handed the run's own coordinates and lattice either way.
EXACT_FRAMES = (2, 3, 63, 64, 65, 128, 512)


def check_frame(info, lattice, x, x2, xyz, n_images, n_fixed=0):
    """The set-up's info against LATTICES[lattice] and the run's coordinates (x, x2) against the model's: see EXACT_FRAMES."""
    opt, box, dims, origin, spacing = LATTICES[lattice]
    assert list(info.dims) == dims
    assert np.array_equal(x2, x)                                # the lattice's first transform: zero coefficients
    if n_images in EXACT_FRAMES and n_fixed <= 1:
        assert list(info.origin) == origin and list(info.spacing) == spacing
        assert np.array_equal(x, xyz)
    else:
        assert np.abs(x.astype(np.float64) - xyz).max() <= 2.0 ** -12
        assert np.abs(np.array(info.origin) - origin).max() <= 2.0 ** -11 and np.abs(np.array(info.spacing) / spacing - 1).max() <= 1e-6

def links_per_point(point_offset, blocks):
    """Number of links of every point: with all weights 1 its weight sum (sWeight) after a deformable sweep."""
    n = np.zeros(int(point_offset[-1]), np.int64)
    for i, j, p, q in blocks:
        np.add.at(n, point_offset[i] + p.astype(np.int64), 1)
        np.add.at(n, point_offset[j] + q.astype(np.int64), 1)
    return n


def link_lengths(point_offset, blocks, xyz):
    x = np.asarray(xyz, np.float32).astype(np.float64)
    return np.concatenate([np.sqrt(np.sum((x[point_offset[i] + p.astype(np.int64)] - x[point_offset[j] + q.astype(np.int64)]) ** 2, axis=1))
                           for i, j, p, q in blocks])


def slots(x, lat, brick):
    """{brick (bx, by, bz): scatter blocks} of one image's points x for bricks of brick^3 cells: ceil(points / SCATTER_CHUNK)
    (k_grid.hip.h brick_chunks_kernel), the sort's brick from lattice_design.brick_of."""
    b, count = np.unique(ld.brick_of(x, lat, brick), axis=0, return_counts=True)
    return {tuple(int(v) for v in k): int(-(-c // SCATTER_CHUNK)) for k, c in zip(b, count)}


def check_slots(x, lat, lattice):
    """The scatter blocks of image 0's or image 1's points x on LATTICES[lattice], for either brick edge: the arms are whole
    bricks of 5, 6 and 2 slots, every other brick has one -- but for the edge 8 at spacing 16, where the image is one brick of
    11 slots (three trips of the four-at-a-time loop, two live entries in the last)."""
    for brick in (4, 8):
        s = slots(x, lat, brick)
        if lattice == "narrow" and brick == 8:
            assert s == {(0, 0, 0): 11} and trips(11) == (3, 2)
            continue
        far = max(k[0] for k in s)
        arm = {0: (far, 0, 0), 1: (0, far, 0), 2: (0, 0, far)}
        assert {axis: s[arm[axis]] for axis in ARMS} == ARM_SLOTS, (lattice, brick, s)
        assert all(v == 1 for k, v in s.items() if k not in arm.values()) and (far, far, far) in s, (lattice, brick, s)
    assert trips(5) == (1, 4) and trips(6) == (2, 1) and trips(2) == (1, 1)


def trips(n_slots):
    """(trips of lattice_step_kernel's four-at-a-time loop over the slots behind the first, live entries of the last trip)."""
    rest = n_slots - 1
    return -(-rest // 4), (rest - 1) % 4 + 1 if rest else 0


def active(lat, point_offset, xyz):
    """[images, n_cp] bool: the (image, node) pairs some point of the image reaches -- the nodes of the 4^3 stencil of the cell
    the scatter finds (f32 quotient) or the transform finds (f64 quotient), all points, linked or not: the sparse form's
    active pairs (k_grid.hip.h lattice_mask_kernel).  Every other pair of a node holds the node's shared value."""
    n_img = len(point_offset) - 1
    out = np.zeros((n_img, lat.n_cp), bool)
    o = np.arange(-1, 3)
    for i in range(n_img):
        x = xyz[point_offset[i]:point_offset[i + 1]]
        for cell in (ld.cells32(x, lat)[0], ld.cells64(x, lat)[0]):
            gx, gy, gz = (cell[:, k, None] + o for k in range(3))
            ok = ((gz >= 0) & (gz < lat.dims[2]))[:, :, None, None] & ((gy >= 0) & (gy < lat.dims[1]))[:, None, :, None] \
                & ((gx >= 0) & (gx < lat.dims[0]))[:, None, None, :]
            node = gx[:, None, None, :] + lat.dims[0] * (gy[:, None, :, None] + lat.dims[1] * gz[:, :, None, None])
            out[i, node[ok]] = True
    return out


def oversize(coeffs, limit):
    """Number of coefficients beyond the guard's limit: (double) fabsf(c) > limit[axis], strictly (imageGroup.cxx:425).
    coeffs f32 [images, n_cp, 3], limit f64 [3]."""
    c = np.asarray(coeffs)
    assert c.dtype == np.float32 and c.shape[-1] == 3
    return int(np.count_nonzero(np.abs(c).astype(np.float64) > np.asarray(limit, np.float64)))


def energy(point_offset, blocks, xyz2, first_image=0):
    """sqrt(sum d^2 / count) over the HALF-links of the images from first_image on, every weight 1, in f64: a link between two
    moving images counts twice, a link to a fixed image once."""
    x = np.asarray(xyz2, np.float32).astype(np.float64)
    total, count = 0.0, 0
    for i, j, p, q in blocks:
        d = x[point_offset[i] + p.astype(np.int64)] - x[point_offset[j] + q.astype(np.int64)]
        halves = int(i >= first_image) + int(j >= first_image)
        total += halves * float(np.sum(d * d)); count += halves * len(p)
    return float(np.sqrt(total / count))


def boundary_ratio(coeffs, spacing=8.0, at="median"):
    """A max_displacement_ratio r whose limit r * spacing IS an attained |coefficient| v (spacing a power of two: the division
    is exact).  at = "median": the attained value nearest the median of the non-zero |c|; "max": the largest.  Returns
    (r f32, v f64, entries with |c| == v)."""
    a = np.abs(np.asarray(coeffs, np.float32)).ravel()
    a = a[a > 0]
    v = a.max() if at == "max" else a[np.argmin(np.abs(a.astype(np.float64) - float(np.median(a))))]
    r = np.float32(float(v) / spacing)
    assert float(r) * spacing == float(v)                    # (double) r * spacing is v, to the bit
    return r, float(v), int(np.count_nonzero(a == v))


def node_class(act, node, arm_nodes):
    """For the record of where the largest err / bound sits."""
    k, n = int(act[:, node].sum()), act.shape[0]
    return f"a node {k} of {n} images reach" + (", under a filled arm" if arm_nodes[node] else "")
