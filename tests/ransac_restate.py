"""The RANSAC stage's census and selection restated in NumPy (frog_amd/csrc/device/k_ransac.hip.h, frog_ransac in
frog_hip.hip; upstream imageGroup.cxx:629-804), and the designed groups the RANSAC tests share.

One candidate's census: every half-link of the image, own point's xyz through the candidate as vtkLinearTransform does for
a float point -- f64 row sums ((m0 x + m1 y) + m2 z) + m3 rounded to f32 --, f32 squared distance (dx dx + dy dy) + dz dz to
the partner's xyz2, strict `<` against (float)pow((double)inlier_distance, 2).  NumPy's element-wise operations round after
every multiplication and addition, as the device code built with -ffp-contract=off does, so counts are compared with ==."""
import numpy as np

from frog_amd.pairs import Pairs

F4, F8 = np.float32, np.float64


def half_links(pairs, image):
    """(owner, partner): global point index of the own point and of the partner of every half-link of `image`, in the
    link table's order."""
    po, rp = np.asarray(pairs.point_offset, np.int64), np.asarray(pairs.row_ptr, np.int64)
    pb, pe = po[image], po[image + 1]
    owner = np.repeat(np.arange(pb, pe), np.diff(rp[pb:pe + 1]))
    l0, l1 = rp[pb], rp[pe]
    partner = po[np.asarray(pairs.link_image[l0:l1], np.int64)] + np.asarray(pairs.link_point[l0:l1], np.int64)
    return owner, partner


def max_distance2(inlier_distance):
    with np.errstate(over="ignore"):
        return F4(F8(F4(inlier_distance)) ** 2)


def inliers(candidate, xyz, xyz2, owner, partner, inlier_distance):
    """bool per half-link: the candidate (12 doubles, rows 0..2 of the matrix) brings it within the distance."""
    m = np.asarray(candidate, F8).reshape(3, 4)
    a = np.asarray(xyz, F4)[owner].astype(F8)
    with np.errstate(all="ignore"):
        t = (((m[:, 0] * a[:, 0:1] + m[:, 1] * a[:, 1:2]) + m[:, 2] * a[:, 2:3]) + m[:, 3]).astype(F4)
        d = t - np.asarray(xyz2, F4)[partner]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        assert d2.dtype == F4
        return d2 < max_distance2(inlier_distance)


def census(candidates, xyz, xyz2, owner, partner, inlier_distance):
    cand = np.asarray(candidates, F8).reshape(-1, 12)
    return np.array([inliers(c, xyz, xyz2, owner, partner, inlier_distance).sum() for c in cand], np.uint32)


def select(counts, usable, batches):
    """(best census, winner or -1): the first strictly larger usable count within a batch, then the first strictly larger
    batch maximum in batch order."""
    per = len(counts) // batches
    best, winner = 0, -1
    for b in range(batches):
        batch_max, batch_best = 0, -1
        for c in range(b * per, (b + 1) * per):
            if usable[c] and counts[c] > batch_max:
                batch_max, batch_best = int(counts[c]), c
        if batch_max > best:
            best, winner = batch_max, batch_best
    return best, winner


# ---- designed groups ------------------------------------------------------------------------------------------------------
def designed_group(degrees, image=1, n_images=3, n_partner=37, seed=0, duplicate=1):
    """Image `image` has len(degrees) points, point p with degrees[p] * duplicate half-links (each link `duplicate` times)
    to random points of the other images; the others have n_partner points and are linked p <-> p among themselves."""
    rng = np.random.default_rng(seed)
    degrees = np.asarray(degrees, np.int64)
    sizes = np.full(n_images, n_partner)
    sizes[image] = len(degrees)
    po = np.concatenate([[0], np.cumsum(sizes)])
    xyz = rng.uniform(-100, 100, (po[-1], 3)).astype(F4)
    others = [j for j in range(n_images) if j != image]
    own = np.repeat(np.repeat(np.arange(len(degrees)), degrees), duplicate).astype(np.uint32)
    to_image = np.repeat(rng.choice(others, int(degrees.sum())), duplicate)
    to_point = np.repeat(rng.integers(0, n_partner, int(degrees.sum())), duplicate).astype(np.uint32)
    blocks = []
    for j in others:
        sel = to_image == j
        if sel.any():
            blocks.append((image, j, own[sel], to_point[sel]) if image < j else (j, image, to_point[sel], own[sel]))
    idx = np.arange(n_partner, dtype=np.uint32)
    blocks += [(i, j, idx, idx) for i in others for j in others if i < j]
    return Pairs.from_arrays(po, xyz, blocks)


def quaternion_matrix(q):
    w, x, y, z = np.asarray(q, F8) / np.linalg.norm(q)
    return np.array([[w*w + x*x - y*y - z*z, 2 * (x*y - w*z), 2 * (x*z + w*y)],
                     [2 * (x*y + w*z), w*w - x*x + y*y - z*z, 2 * (y*z - w*x)],
                     [2 * (x*z - w*y), 2 * (y*z + w*x), w*w - x*x - y*y + z*z]])


def similarity(q, s, t):
    m = np.eye(4)
    m[:3, :3] = s * quaternion_matrix(q)
    m[:3, 3] = t
    return m


def planted_group(moving, transforms, member, extra_unlinked=0, links=None, noise=0.0):
    """Two images: image 0 fixed, image 1 the measured one with the points `moving` (n, 3) (+ extra_unlinked points without
    links at its end).  Point p's partner in image 0 lies at transforms[member[p]] applied to it (+ Gaussian noise), so
    without noise the half-links of the members of one transform are fitted exactly (to float32 rounding) by it.
    links: the moving points that get a link, in order, repeats allowed (default: each once)."""
    moving = np.asarray(moving, F8)
    n = len(moving)
    rng = np.random.default_rng(99)
    target = np.stack([transforms[k][:3, :3] @ p + transforms[k][:3, 3] for p, k in zip(moving, member)])
    target = target + rng.normal(0, noise, target.shape) if noise else target
    links = (np.arange(n) if links is None else np.asarray(links)).astype(np.uint32)
    xyz = np.concatenate([target, moving, rng.uniform(-100, 100, (extra_unlinked, 3))]).astype(F4)
    return Pairs.from_arrays(np.array([0, n, 2 * n + extra_unlinked], np.uint32), xyz, [(0, 1, links, links)])


def sparse_group(noise=1.0, seed=5):
    """The sparsely linked image: 40 points of which 5 have a link (one of them two, a duplicate), to a copy of themselves
    under a planted similarity plus noise.  Of the four-correspondence draws on it about a quarter hold two distinct
    correspondences or fewer (undetermined: a line).  Returns (pairs, planted matrix)."""
    moving = np.random.default_rng(seed).uniform(-80, 80, (5, 3))
    T = similarity((0.9, 0.2, -0.3, 0.1), 1.2, (15.0, -8.0, 4.0))
    return planted_group(moving, [T], [0] * 5, extra_unlinked=35, links=[0, 1, 2, 2, 3, 4], noise=noise), T
