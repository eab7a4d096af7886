"""Groups of images whose every half-link weighs exactly 1 or exactly +0 and whose every product and sum is exact in the
precision it is formed in, and an order-free f64 restatement of what the three half-link sweeps (k_links.hip.h: linear,
deformable, counting) make of them -- per-point sums, energies, census, the matrices after one linear step, the length of a
culling list.  One dropped, doubled or mis-attributed half-link changes an integer, so every comparison is `==`
(tests/test_links_design.py on the CPU oracle, tests/test_gpu_links_design.py on the device in every form of the sweep).

Coordinates.  Multiples of 1/64 in [0, 64]: at most 13 significant bits, 12 below 64, so pa.x * pa.x is exact in f32 and every
difference of two coordinates is exact.  Every image begins with the frame (0,0,0), (64,64,64), as in lattice_design.py: all
bounding boxes are equal and the linear initialisation is the identity up to the rounding of an f32 average
(linear_init_translation: exactly the identity for 3 and 9 images); the tests hand both coordinate sets in.

Sites.  Points sit on SITES that come in pairs (s, s ^ 1): the mate of a site lies 31 or 40 along x, or 58 along every axis
(d = 100.46), away.  A point is its site moved by -1, 0 or +1 sixty-fourths per axis.
  near link   two points of one site in two images: at most 2/64 apart per axis, d2 <= 3 (2/64)^2 = 0.0029 < 0.01 (D2_FIX): the
              `d < 0.1` rule of stats.h:87, which every form of the weight has, makes the weight exactly 1;
  far link    a point and a point of the mate site: d >= 30.96.  Under the mixture EM = (1, 20, 0.5) of every image
              (d / c1)^2 / 2 >= 479, so the inlier term is below 2^-690: +0 in f32 in the fast form (inlier_probability: v_exp_f32
              flushes, kq1 (d2 0) = 0, 0 / (x2 + eps) = +0), in the one-exponential form (inlier_weight_pair: the exponent is above
              600, the exponential overflows, rcp(inf) = 0) and in the exact form (inlier_probability_exact: the f64 product with
              exp(-479) cast to f32 is 0).  An outlier in the deformable and counting sweeps, +0 in every sum of the linear one.
No link of any other kind exists: `expected` counts the links that are neither and the tests assert 0.
The far distances: 31 (behind the certified cutoff of 4.5, inside the deformable list's skin of 2 x + 25: listed, weight 0), 40
(beyond the list cutoff of 34: not listed) and 100.46.  All of them are beyond the linear stage's list cutoff (28.6).

Exactness.  Deformable sums: w2 dx is a multiple of 1/64 of at most 2/64, a point has at most 1000 near links, so its sums stay
below 2^11 in 1/64ths and its count below 2^11: f32 holds them.  d2 of a near link is a multiple of 2^-12 below 2^-8: exact
in f32, the f64 sums are exact.  Linear sums:
f32 products of a 12-bit coordinate with itself, f64 sums of multiples of 2^-12 below 2^41; fl32(fl32(sqrt d2)^2) is a multiple
of 2^-35 below 2^-8.  The variance terms sWeight sPos2 - sPos^2 of linear_update_kernel are exact as long as an image has fewer
than 2^14 half-links (`expected` checks the products in integers): no rounding, whatever the order or the contraction.  What is
left is IEEE f64 arithmetic on exact inputs, restated operation by operation, and one pow, which the CPU test keeps away from
the midpoints of f32.

The classes (counted by `classes`, asserted by the CPU test):
  tiles         images of 0, 1, 253, 254, 255 and 510 points besides the frame -- tiles of 2, 3, 255, 256, 257 = 256 + 1 and
                512 = two full tiles -- and images of several thousand points (group "g3": 12 and 11 tiles);
  image counts  "g3": 3 images, five empty partner groups; "g9", "g24": every partner group non-empty, steps that span several
                partner images; "g300": dozens of images per group; "g2100": groups wider than 256 images, which forces the wide
                record form and the constants read from memory;
  ranges        records per (tile, partner group) of 0, 1, 63, 64, 65 (a sweep step), 127, 128, 129 (REC_CHUNK), 383, 384, 385
                (BODY_STEPS steps) and 4500 (past the 64 steps of STEP_WINDOW) in "g24", whose images are one tile each: image
                i < 11 has RANGE_LENGTHS[i] links into partner group 4 + i // 3 and no other; ranges of near links only, of far
                links only, mixed;
  degrees       points without a link, with far links only (sums exactly 0, outliers > 0), of degree 1, 2, 64, 65, a point
                linked 300 times to the same partner, a point with 1000 distinct near partners in one image (coincident points
                of the partner image: only 27 positions lie within +-1/64);
  zero records  (0,0,0) of the first image of a group linked to (0,0,0) of the first image of another group: the frame point
                has the smallest Morton key of its image, so the narrow record of either direction is 0, a padding record's
                value;
  set B         the same links, one image (Group.moved) moved by 40 along x, frame excepted: its points sit on sites whose mate
                is 40 away, so its near links become far and its far links near.  Classes come from distances, not labels.
"""
import numpy as np

F = np.float32
TILE_POINTS, N_GROUPS, STEP, REC_CHUNK, BODY_STEPS, STEP_WINDOW = 256, 8, 64, 128, 6, 64      # ctx.h, k_links.hip.h
EM = (1.0, 20.0, 0.5)                       # every image's (c1, c2, ratio)
UNIT = 64                                   # coordinates are integers / UNIT
NEAR_D2 = 3.0 * (2.0 / UNIT) ** 2           # 0.0029
FAR_D = 30.0
LINEAR_ALPHA, USE_SCALE = 0.5, 1            # imageGroup.h's defaults, frog_options' too
RANGE_LENGTHS = [1, 63, 64, 65, 127, 128, 129, 383, 384, 385, 4500]
GROUPS = ("g3", "g9", "g24", "g300", "g2100")
KINDS = ("x40", "x31", "x40", "diag")       # the site pairs' kinds, in turn


# ---- the layout's counting (prep.h build_layout), restated -------------------------------------------------------------------

def group_begin(po, n_groups=N_GROUPS):
    """First image of every partner group: contiguous image ranges balanced by point count."""
    po = np.asarray(po, np.int64)
    n = len(po) - 1
    return np.array([0] + [int(np.searchsorted(po[:n], int(po[-1]) * g // n_groups, "left")) for g in range(1, n_groups)] + [n])


def group_of(po, n_groups=N_GROUPS):
    gb = group_begin(po, n_groups)
    out = np.zeros(len(po) - 1, np.int64)
    for g in range(n_groups):
        out[gb[g]:gb[g + 1]] = g
    return out


# ---- building ----------------------------------------------------------------------------------------------------------------

def _site_pairs(rng, kinds, n_pairs):
    """[2 n_pairs, 3] integer coordinates: site 2 m and its mate 2 m + 1; every site at least 1 from the box's faces."""
    out = np.empty((2 * n_pairs, 3), np.int64)
    for m in range(n_pairs):
        kind = kinds[m % len(kinds)]
        if kind == "diag":
            s0 = rng.integers(1 * UNIT, 5 * UNIT + 1, 3)
            s1 = s0 + 58 * UNIT
        else:
            reach = 40 if kind == "x40" else 31
            s0 = np.array([rng.integers(1 * UNIT, (63 - reach) * UNIT + 1), rng.integers(1 * UNIT, 63 * UNIT + 1), rng.integers(1 * UNIT, 63 * UNIT + 1)])
            s1 = s0 + np.array([reach * UNIT, 0, 0])
        out[2 * m], out[2 * m + 1] = s0, s1
    return out


class _Image:
    def __init__(self, rng, sites, site_ids, reserved=()):
        ids = np.asarray(site_ids, np.int64)
        pts = sites[ids] + rng.integers(-1, 2, (len(ids), 3)) if len(ids) else np.zeros((0, 3), np.int64)
        self.units = np.concatenate([np.array([[0, 0, 0], [64 * UNIT] * 3], np.int64), pts])
        self.site = np.concatenate([[-1, -1], ids])             # per local point; the frame has none
        self.generic = np.ones(len(self.site), bool)            # may take part in the random links
        self.generic[:2] = False
        for t in reserved:
            self.generic[2 + t] = False
        self._by_site = None

    def by_site(self):
        if self._by_site is None:
            self._by_site = {}
            for q in np.nonzero(self.generic)[0]:
                self._by_site.setdefault(int(self.site[q]), []).append(int(q))
        return self._by_site


def _candidates(a, b, far):
    """Every (p in a, q in b), both generic, with q on p's site (far = 0) or on its mate (far = 1)."""
    ps, qs = [], []
    by = b.by_site()
    for p in np.nonzero(a.generic)[0]:
        for q in by.get(int(a.site[p]) ^ far, ()):
            ps.append(int(p)); qs.append(q)
    return np.array(ps, np.int64), np.array(qs, np.int64)


class _Links:
    def __init__(self):
        self.d = {}

    def add(self, i, p, j, q):
        """Links point p of image i -- point q of image j (local indices, arrays; a pair may come more than once)."""
        p, q = np.atleast_1d(np.asarray(p, np.int64)), np.atleast_1d(np.asarray(q, np.int64))
        assert i != j and len(p) == len(q)
        if i > j:
            i, p, j, q = j, q, i, p
        e = self.d.setdefault((i, j), ([], []))
        e[0].append(p); e[1].append(q)

    def pick(self, rng, images, i, j, n_near, n_far):
        for far, n in ((0, n_near), (1, n_far)):
            p, q = _candidates(images[i], images[j], far)
            if n and len(p):
                k = rng.choice(len(p), size=min(n, len(p)), replace=False)
                self.add(i, p[k], j, q[k])


class Group:
    """name, po [n + 1], xyz / xyz_b (f32 [P, 3]: coordinate sets A and B), blocks (Pairs.from_arrays' form), a / b (global
    indices of every link's two points, a in the lower image), image_a / image_b, moved (the image set B moves), marks (name ->
    global point index of the designed degrees)."""

    def __init__(self, name, images, links, moved, marks):
        self.name, self.moved, self.marks = name, moved, marks
        self.po = np.concatenate([[0], np.cumsum([len(im.units) for im in images])]).astype(np.int64)
        units = np.concatenate([im.units for im in images])
        assert units.min() >= 0 and units.max() <= 64 * UNIT
        self.xyz = (units / UNIT).astype(F)
        ub = units.copy()
        ub[self.po[moved] + 2:self.po[moved + 1], 0] += 40 * UNIT
        assert ub.max() <= 64 * UNIT
        self.xyz_b = (ub / UNIT).astype(F)
        assert np.array_equal(self.xyz.astype(np.float64) * UNIT, units) and np.array_equal(self.xyz_b.astype(np.float64) * UNIT, ub)
        self.blocks = []
        a, b, ia, ib = [], [], [], []
        for (i, j) in sorted(links.d):                          # i-major, j ascending: the order `match` writes
            p, q = np.concatenate(links.d[(i, j)][0]), np.concatenate(links.d[(i, j)][1])
            order = np.argsort(p, kind="stable")
            p, q = p[order], q[order]
            self.blocks.append((i, j, p.astype(np.uint32), q.astype(np.uint32)))
            a.append(self.po[i] + p); b.append(self.po[j] + q)
            ia.append(np.full(len(p), i)); ib.append(np.full(len(p), j))
        self.a, self.b = np.concatenate(a), np.concatenate(b)
        self.image_a, self.image_b = np.concatenate(ia), np.concatenate(ib)
        self.n_images, self.n_points = len(images), int(self.po[-1])
        self.group_begin = group_begin(self.po)
        self.group_of = group_of(self.po)

    @property
    def n_half_links(self):
        return 2 * len(self.a)

    def coordinates(self, which):
        return self.xyz if which == "A" else self.xyz_b

    def em_table(self):
        return np.tile(np.array(EM, F), (self.n_images, 1))

    def image_of(self, point):
        return int(np.searchsorted(self.po, point, "right") - 1)


def _zero_records(links, po):
    """(0,0,0) -- (0,0,0) between the first images of the non-empty groups, two by two (an odd one out with its neighbour)."""
    gb = group_begin(po)
    firsts = [int(gb[g]) for g in range(N_GROUPS) if gb[g + 1] > gb[g]]
    pairs = [(firsts[k], firsts[k + 1]) for k in range(0, len(firsts) - 1, 2)]
    if len(firsts) % 2 and len(firsts) > 1:
        pairs.append((firsts[-2], firsts[-1]))
    for i, j in pairs:
        links.add(i, [0], j, [0])
    return pairs


def _po_of(images):
    return np.concatenate([[0], np.cumsum([len(im.units) for im in images])])


def _moved_sites(n, n_pairs, kinds=KINDS):
    """n site ids for the image that set B moves: sites whose mate is 40 along x, in turn (`kinds`: what _site_pairs was given)."""
    s0 = [2 * m for m in range(n_pairs) if kinds[m % len(kinds)] == "x40"]
    return [s0[k % len(s0)] for k in range(n)]


def _build_g3(rng):
    """3 images: 3000 + 4 specials, 1500 + the clusters, 510 (set B's).  Five partner groups are empty."""
    n_pairs = 1500 + 4
    sites = _site_pairs(rng, KINDS, n_pairs)
    hub, d64, d65, dup = (2 * (1500 + k) for k in range(4))             # four sites of their own
    reserved = list(range(560, 600))
    im0 = _Image(rng, sites, list(range(3000)) + [hub, d64, d65, dup], reserved=reserved + [3000, 3001, 3002, 3003])
    cluster = [hub] * 1000 + [d64] * 64 + [d65] * 65 + [dup]
    im1 = _Image(rng, sites, list(range(1500)) + cluster, reserved=range(1500, 1500 + len(cluster)))
    im2 = _Image(rng, sites, _moved_sites(510, 1500))
    images = [im0, im1, im2]
    L = _Links()
    L.pick(rng, images, 0, 1, 1400, 1200)
    L.pick(rng, images, 0, 2, 450, 400)
    L.pick(rng, images, 1, 2, 300, 250)
    first = 2 + 1500                                                    # image 1's first cluster point
    L.add(0, np.full(1000, 2 + 3000), 1, first + np.arange(1000))       # 1000 distinct near partners
    L.add(0, np.full(64, 2 + 3001), 1, first + 1000 + np.arange(64))
    L.add(0, np.full(65, 2 + 3002), 1, first + 1064 + np.arange(65))
    L.add(0, np.full(300, 2 + 3003), 1, np.full(300, first + 1129))     # one link, 300 times
    for t in range(580, 590):                                           # far links only: one, two or three
        for k in range(1 + t % 3):
            L.add(0, [2 + t], 1, [2 + (t ^ 1)])
    for t in range(570, 580):                                           # degree 1
        L.add(0, [2 + t], 1, [2 + t])
    for t in range(560, 570):                                           # degree 2: one near, one far
        L.add(0, [2 + t], 1, [2 + t])
        L.add(0, [2 + t], 1, [2 + (t ^ 1)])
    po = _po_of(images)
    _zero_records(L, po)
    marks = {"hub": 2 + 3000, "degree64": 2 + 3001, "degree65": 2 + 3002, "duplicate300": 2 + 3003,
             "no_link": 2 + 595, "far_only": 2 + 585, "degree1": 2 + 575, "degree2": 2 + 565}
    return Group("g3", images, L, 2, marks)


# points: + 2 each.  Partner groups {0} {1} {2} {3} {4, 5} {6} {7} {8}: the frame-only image begins a group, the image of 3 points is one
G9_EXTRAS = [254, 233, 253, 229, 0, 255, 1, 214, 195]


def _build_g9(rng):
    """9 images of 0, 1, 253, 254, 255, ... points besides the frame; every partner group holds one or two of them."""
    sites = _site_pairs(rng, KINDS, 128)
    moved = 7
    images = [_Image(rng, sites, _moved_sites(n, 128) if i == moved else list(range(n))) for i, n in enumerate(G9_EXTRAS)]
    L = _Links()
    for i in range(9):
        for j in range(i + 1, 9):
            L.pick(rng, images, i, j, 60, 40)
    _zero_records(L, _po_of(images))
    return Group("g9", images, L, moved, {})


def _build_g24(rng):
    """24 images of one full tile each, three per partner group.  Image i < 11 has RANGE_LENGTHS[i] links into partner group
    4 + i // 3 and nothing else but, for the first image of a group, its zero record into the neighbouring group."""
    kinds = ("x40", "x31")
    sites = _site_pairs(rng, kinds, 127)
    moved = 23
    images = [_Image(rng, sites, _moved_sites(254, 127, kinds) if i == moved else list(range(254))) for i in range(24)]
    L = _Links()
    for i, want in enumerate(RANGE_LENGTHS):
        j = 12 + i
        near, far = _candidates(images[i], images[j], 0), _candidates(images[i], images[j], 1)
        assert len(near[0]) == 254 and len(far[0]) == 254
        if want <= 64:
            L.add(i, near[0][:want], j, near[1][:want])         # near only, every point once: no step holds a point twice
        elif want == 65:
            L.add(i, far[0][:want], j, far[1][:want])           # far only
        elif want < 383:
            L.add(i, near[0][:100], j, near[1][:100])
            L.add(i, far[0][:want - 100], j, far[1][:want - 100])
        elif want < 4096:
            L.add(i, near[0], j, near[1])
            L.add(i, far[0][:want - 254], j, far[1][:want - 254])
        else:                                                   # over the three images of the group, every link three times
            assert want % 9 == 0
            per = want // 9
            for jj in (21, 22, 23):
                nr, fr = _candidates(images[i], images[jj], 0), _candidates(images[i], images[jj], 1)
                p = np.concatenate([nr[0], fr[0]])[:per]
                q = np.concatenate([nr[1], fr[1]])[:per]
                assert len(p) == per, (jj, len(p))
                for _ in range(3):
                    L.add(i, p, jj, q)
    _zero_records(L, _po_of(images))
    return Group("g24", images, L, moved, {})


def _build_g300(rng):
    """300 images of 6 .. 10 points: 37 or 38 images per partner group."""
    sites = _site_pairs(rng, KINDS, 4)
    moved = 150
    extras = rng.integers(4, 9, 300)
    images = [_Image(rng, sites, _moved_sites(n, 4) if i == moved else list(range(n))) for i, n in enumerate(extras)]
    L = _Links()
    seen = set()
    partners = list(rng.integers(0, 300, (1500, 2))) + [(moved, j) for j in range(0, 300, 7)]
    for i, j in partners:
        i, j = int(min(i, j)), int(max(i, j))
        if i == j or (i, j) in seen:
            continue
        seen.add((i, j))
        L.pick(rng, images, i, j, int(rng.integers(1, 4)), int(rng.integers(0, 3)))
    _zero_records(L, _po_of(images))
    return Group("g300", images, L, moved, {})


def _build_g2100(rng):
    """2100 images of 3 or 4 points: partner groups of more than 256 images."""
    sites = _site_pairs(rng, ("x40", "x31"), 2)
    moved = 1000
    images = []
    for i in range(2100):
        n = int(rng.integers(1, 3))
        base = 0 if i == moved else 2 * (i % 2)
        images.append(_Image(rng, sites, [base] * n if i == moved else [base + k for k in range(n)]))
    L = _Links()
    seen = set()
    partners = list(rng.integers(0, 2100, (4000, 2))) + [(moved, j) for j in range(0, 2100, 20)]
    for i, j in partners:
        i, j = int(min(i, j)), int(max(i, j))
        if i == j or (i, j) in seen:
            continue
        seen.add((i, j))
        L.pick(rng, images, i, j, int(rng.integers(1, 3)), int(rng.integers(0, 2)))
    _zero_records(L, _po_of(images))
    return Group("g2100", images, L, moved, {})


SEEDS = {"g3": 3, "g9": 9, "g24": 24, "g300": 300, "g2100": 2100}
_groups, _pairs = {}, {}


def build(name):
    """The designed group `name` (one of GROUPS), built once."""
    if name not in _groups:
        rng = np.random.default_rng(SEEDS[name])
        _groups[name] = {"g3": _build_g3, "g9": _build_g9, "g24": _build_g24, "g300": _build_g300, "g2100": _build_g2100}[name](rng)
    return _groups[name]


def pairs(name):
    """The group as frog_amd.pairs.Pairs (built once)."""
    from frog_amd.pairs import Pairs
    if name not in _pairs:
        g = build(name)
        _pairs[name] = Pairs.from_arrays(g.po, g.xyz, g.blocks)
        assert _pairs[name].n_half_links == g.n_half_links
    return _pairs[name]


# ---- the half-links, and what they are ---------------------------------------------------------------------------------------

def half_links(group, xyz2):
    """Every half-link, both directions of every link: own point, partner point, own image, partner image, the exact
    difference partner - own (f64 [n, 3]), its exact squared length and the sweep's f32 d2 (dx dx + dy dy + dz dz, product by
    product)."""
    x = np.asarray(xyz2, F)
    own = np.concatenate([group.a, group.b]); other = np.concatenate([group.b, group.a])
    img = np.concatenate([group.image_a, group.image_b]); img_o = np.concatenate([group.image_b, group.image_a])
    d = x[other].astype(np.float64) - x[own].astype(np.float64)
    d32 = x[other] - x[own]
    assert np.array_equal(d32.astype(np.float64), d)            # differences of multiples of 1/64 below 128: exact in f32
    with np.errstate(all="ignore"):
        d2_32 = ((d32[:, 0] * d32[:, 0]).astype(F) + (d32[:, 1] * d32[:, 1]).astype(F)).astype(F) + (d32[:, 2] * d32[:, 2]).astype(F)
    return dict(own=own, other=other, image=img, image_other=img_o, d=d, d2=(d * d).sum(axis=1), d2_f32=d2_32.astype(F))


def listed(d2_f32, cut_a, cut_b):
    """cull_build_kernel's criterion (k_cull.hip.h; the list-writing sweep has the same): a half-link is left out when
    d2 >= min(cutA, cutB)^2 in f32 and d2 is finite."""
    with np.errstate(all="ignore"):
        cut = np.minimum(np.asarray(cut_a, F), np.asarray(cut_b, F))
        return ~((d2_f32 >= (cut * cut).astype(F)) & (d2_f32 < F(np.inf)))


def linear_init_translation(n_images):
    """The translation the linear initialisation gives every image of a group whose bounding boxes are all [0, 64]^3
    (imageGroup.cxx:823-824): the images' anchors, 32, are averaged in f32 as n terms fl(32 / n), and each image is moved by
    that average minus its anchor.  Exactly 0 for 3 and 9 images, 4e-6 for 24 and -4e-4 for 2100 -- which is why the tests hand
    the coordinates in (set_points2 / set_xyz2) and take the matrices the linear step starts from as they are."""
    term, avg = F(F(32.0) / F(n_images)), F(0)
    for _ in range(n_images):
        avg = F(avg + term)
    return float(F(avg - F(32.0)))


def linear_update(sums, t0=0.0, alpha=LINEAR_ALPHA, use_scale=USE_SCALE):
    """linear_update_kernel (imageGroup.cxx:1123-1143) from the matrices of the linear initialisation (scale 1, translation t0
    on every axis), operation by operation: sums [n, 18] f64 -> (scale [n, 3], translation [n, 3], the f64 powers [n, 3])."""
    n = len(sums)
    t0 = float(F(t0))
    scale, trans, power = np.ones((n, 3)), np.full((n, 3), t0), np.full((n, 3), np.nan)
    la = np.float64(F(alpha))
    with np.errstate(all="ignore"):
        for k in range(3):
            sDisp, sPosA, sPosB = sums[:, k], sums[:, 3 + k], sums[:, 6 + k]
            sPosA2, sPosB2, sW = sums[:, 9 + k], sums[:, 12 + k], sums[:, 15]
            new = np.ones(n, F)
            if use_scale:
                power[:, k] = np.power((sW * sPosB2 - sPosB * sPosB) / (sW * sPosA2 - sPosA * sPosA), 0.5 * la)
                new = power[:, k].astype(F)
            ok = ~np.isnan(new)
            s = (F(1.0) * new).astype(F).astype(np.float64)
            t = t0 + la * sDisp / sW + sPosA * (F(1) - new).astype(F).astype(np.float64) / sW
            scale[:, k] = np.where(ok, s, 1.0)
            trans[:, k] = np.where(ok, t, t0)
    return scale, trans, power


def expected(group, xyz2, cut_list=None):
    """What the sweeps must make of `group` at the coordinates xyz2, in f64 and in no particular order.  A dict:
      sums         f32 [P, 4]: per point the sum of (partner - own) over its near half-links and their number
      e_d2, e_n    f64 [n_images]: per image the sum of d2 and the number of its near half-links (deformable E over a set of
                   images: sqrt(sum e_d2 / sum e_n));  E: over all images
      inliers, outliers   int [n_images]: the census
      l_d2, l_n    the same for the linear E: terms fl32(fl32(sqrt d2)^2);  E_linear over all images
      linear_sums  f64 [n_images, 18]: the linear sweep's sums per image;  scale, translation [n_images, 3] after one linear step
                   from the linear initialisation (translation t0 on every axis: linear_init_translation), power
      near, far, other    numbers of half-links;  listed: with cut_list (f32 per image), the half-links a list holds
    """
    h = half_links(group, xyz2)
    nI, P = group.n_images, group.n_points
    near = h["d2"] <= NEAR_D2
    far = h["d2"] >= FAR_D ** 2
    out = dict(near=int(near.sum()), far=int(far.sum()), other=int((~near & ~far).sum()))
    own, img = h["own"][near], h["image"][near]
    sums = np.zeros((P, 4))
    for k in range(3):
        sums[:, k] = np.bincount(own, weights=h["d"][near, k], minlength=P)
    sums[:, 3] = np.bincount(own, minlength=P)
    out["sums"] = sums.astype(F)
    assert np.array_equal(out["sums"].astype(np.float64), sums)
    out["degree"] = np.bincount(h["own"], minlength=P)
    out["e_d2"] = np.bincount(img, weights=h["d2"][near], minlength=nI)
    out["e_n"] = np.bincount(img, minlength=nI).astype(np.float64)
    out["inliers"] = np.bincount(img, minlength=nI)
    out["outliers"] = np.bincount(h["image"][~near], minlength=nI)
    d32 = np.sqrt(h["d2_f32"][near])                            # f32, correctly rounded
    assert np.array_equal(h["d2_f32"][near].astype(np.float64), h["d2"][near])
    term = (d32 * d32).astype(F).astype(np.float64)
    out["l_d2"] = np.bincount(img, weights=term, minlength=nI)
    out["l_n"] = out["e_n"]
    with np.errstate(all="ignore"):
        out["E"] = float(np.sqrt(out["e_d2"].sum() / out["e_n"].sum()))
        out["E_linear"] = float(np.sqrt(out["l_d2"].sum() / out["l_n"].sum()))
    # the linear sweep's 18 sums: sDisp3 sPosA3 sPosB3 sPosA2_3 sPosB2_3 sWeight (sDistances sWeights)
    x = np.asarray(xyz2, F).astype(np.float64)
    pa, pb = x[own], x[h["other"][near]]
    ls = np.zeros((nI, 18))
    for k in range(3):
        for col, v in ((k, h["d"][near, k]), (3 + k, pa[:, k]), (6 + k, pb[:, k]), (9 + k, pa[:, k] * pa[:, k]), (12 + k, pb[:, k] * pb[:, k])):
            ls[:, col] = np.bincount(img, weights=v, minlength=nI)
    ls[:, 15], ls[:, 16], ls[:, 17] = out["e_n"], out["l_d2"], out["l_n"]
    out["linear_sums"] = ls
    # exactness of the variance terms, in integers: sW sPos2 and sPos^2 in units of 2^-12 stay below 2^53
    big = 0
    for i in range(nI):
        for col in (3, 6):
            for k in range(3):
                s1, s2 = int(round(ls[i, col + k] * UNIT)), int(round(ls[i, col + 6 + k] * UNIT * UNIT))
                big = max(big, int(ls[i, 15]) * s2, s1 * s1)
    out["variance_bits"] = big.bit_length()
    out["t0"] = linear_init_translation(nI)
    out["scale"], out["translation"], out["power"] = linear_update(ls, out["t0"])
    if cut_list is not None:
        cut = np.asarray(cut_list, F)
        out["listed"] = int(listed(h["d2_f32"], cut[h["image"]], cut[h["image_other"]]).sum())
    return out


# ---- the classes -------------------------------------------------------------------------------------------------------------

def range_lengths(group):
    """Records per (tile, partner group) for the images of ONE tile, where tile membership is trivial: int [n_images, N_GROUPS],
    -1 in the rows of larger images.  Also per range the near and the far half-links at coordinate set A."""
    h = half_links(group, group.xyz)
    nI = group.n_images
    key = h["image"] * N_GROUPS + group.group_of[h["image_other"]]
    near = h["d2"] <= NEAR_D2
    total = np.bincount(key, minlength=nI * N_GROUPS).reshape(nI, N_GROUPS)
    n_near = np.bincount(key[near], minlength=nI * N_GROUPS).reshape(nI, N_GROUPS)
    one_tile = np.diff(group.po) <= TILE_POINTS
    total = np.where(one_tile[:, None], total, -1)
    return total, n_near, total - n_near


def classes(group):
    """Counters of the designed classes of one group (coordinate set A)."""
    h = half_links(group, group.xyz)
    P = group.n_points
    near = h["d2"] <= NEAR_D2
    degree = np.bincount(h["own"], minlength=P)
    n_near = np.bincount(h["own"][near], minlength=P)
    frame = np.zeros(P, bool)
    frame[group.po[:-1]] = True; frame[group.po[:-1] + 1] = True
    sizes = np.diff(group.po)
    tiles = set()
    for n in sizes:
        tiles.update([TILE_POINTS] * int(n >= TILE_POINTS) + [int(n % TILE_POINTS)] * int(n % TILE_POINTS > 0))
    # multiplicity of a link, distinct near partners of a point inside one partner image
    pair_key = h["own"] * P + h["other"]
    _, mult = np.unique(pair_key, return_counts=True)
    uniq = np.unique(pair_key[near])
    u_own, u_img = uniq // P, np.searchsorted(group.po, uniq % P, "right") - 1
    _, distinct = np.unique(u_own * group.n_images + u_img, return_counts=True)
    gb = group.group_begin
    firsts = set(int(gb[g]) for g in range(N_GROUPS) if gb[g + 1] > gb[g])
    la, lb = group.a - group.po[group.image_a], group.b - group.po[group.image_b]
    zero = (la == 0) & (lb == 0) & np.isin(group.image_a, list(firsts)) & np.isin(group.image_b, list(firsts))
    zero_groups = set(group.group_of[group.image_a[zero]]) | set(group.group_of[group.image_b[zero]])
    total, r_near, r_far = range_lengths(group)
    live = total > 0
    d = np.sqrt(h["d2"][~near])
    return dict(
        images=group.n_images, points=P, half_links=len(h["own"]), near=int(near.sum()), far=int((~near).sum()),
        tiles=tiles, tiles_per_image_max=int(-(-sizes.max() // TILE_POINTS)),
        empty_groups=int(np.count_nonzero(np.diff(gb) == 0)), widest_group=int(np.diff(gb).max()),
        unlinked=int(np.count_nonzero((degree == 0) & ~frame)), far_only=int(np.count_nonzero((degree > 0) & (n_near == 0))),
        degrees=set(int(v) for v in np.unique(degree)), max_multiplicity=int(mult.max()), max_distinct_near_partners=int(distinct.max()),
        zero_records=2 * int(zero.sum()), zero_record_groups=len(zero_groups), non_empty_groups=len(firsts),
        range_lengths=set(int(v) for v in np.unique(total[total >= 0])),
        ranges_near_only=int(np.count_nonzero(live & (r_far == 0))), ranges_far_only=int(np.count_nonzero(live & (r_near == 0))),
        ranges_mixed=int(np.count_nonzero(live & (r_far > 0) & (r_near > 0))),
        far_31=int(np.count_nonzero(d < 32)), far_40=int(np.count_nonzero((d > 39) & (d < 41))), far_100=int(np.count_nonzero(d >= 100)),
        far_min=float(d.min()) if len(d) else np.inf)
