"""The reservoir of the statistics refresh, restated in NumPy, and the tool that designs the inputs of
tests/test_reservoir.py and tests/test_gpu_reservoir.py.

What is restated (k_stats.hip.h select_kernel replays it on the device, oracle/frog_oracle.cpp EmStats::add_sample on the CPU;
this file reads neither):
  * every image owns one mt19937, seeded with 0 once and never reseeded: the stream position carries from refresh to refresh;
  * an image of vs half-links and capacity cap with vs <= cap keeps every ordinal and draws nothing;
  * otherwise half-link k of a refresh draws one word y, u = float32(y) / float32(2**32), and is kept when
    !(u > float32(cap) / float32(vs)); the draw that fills the buffer is the last one of the refresh.

The device consumes the stream in ROUNDS: the words from the saved index to the end of the 624-word state, three per thread
(word q of a round: thread q % 256, row q // 256, lane q % 64).  classify() names, per refresh, where the events of a
replay fall in that layout, so that a test can assert that an input reaches an edge instead of hoping it does.
"""
from fractions import Fraction

import numpy as np

STATE = 624                 # words of one mt19937 state
ROUND_THREADS = 256         # a round tests word q in thread q % 256, row q // 256
WAVE = 64
FIRST_WORD = 2357136044     # std::mt19937 after seed(0)

_stream = np.zeros(0, np.uint32)


def stream(n):
    """The first n words of mt19937 after seed(0)."""
    global _stream
    if len(_stream) < n:
        m = max(n, 2 * len(_stream), 1 << 16)
        raw = np.random.RandomState(0)._bit_generator.random_raw(m)
        assert int(raw[0]) == FIRST_WORD and int(raw.max()) < 2 ** 32
        _stream = raw.astype(np.uint32)
    return _stream[:n]


def uniform(y):
    """(float) rng() / rng.max() of the reference: f32 of the word over f32 of 2^32 - 1, which is 2^32."""
    return np.asarray(y, np.uint32).astype(np.float32) / np.float32(2 ** 32)


def threshold(cap, vs):
    return np.float32(cap) / np.float32(vs)


def replay(vs, cap, refreshes, position=0):
    """Per refresh: (kept ordinals as uint32, stream position before, stream position after)."""
    out = []
    pos = int(position)
    for _ in range(refreshes):
        if vs <= cap:
            out.append((np.arange(vs, dtype=np.uint32), pos, pos))
            continue
        u = uniform(stream(pos + vs)[pos:pos + vs])
        keep = ~(u > threshold(cap, vs))
        count = np.cumsum(keep)
        if count[-1] >= cap:
            used = int(np.searchsorted(count, cap)) + 1      # the draw that fills the buffer is the last one consumed
        else:
            used = vs
        out.append((np.nonzero(keep[:used])[0].astype(np.uint32), pos, pos + used))
        pos += used
    return out


def ordinals(vs, cap, refreshes):
    return [r[0] for r in replay(vs, cap, refreshes)]


def classify(vs, cap, refreshes):
    """Per refresh a dict:
      draws        words consumed (0 on the no-draw path)
      filled       the buffer filled (always False on the no-draw path)
      kept         ordinals kept
      before, after            stream position modulo 624 before and after; `after_index` is the index a replay saves: 624, not
                               0, when the last word consumed was the last of a state
      rounds       rounds of the replay; `states` = states it read words of
      mid_state    the first round starts in the middle of a state (fewer than 624 words left in it)
      q            position within its round of the draw that filled the buffer (None without a fill); row, lane, wave of it
      fill_first_round         that round was the first of the refresh
      fill_round_mid_state     ... and started in the middle of a state
      fill_at_state_end        the filling draw was the last word of a state (saved index 624)
      end_at_state_end         the half-links ran out exactly at a state's end, without a fill (saved index 624)
    """
    out = []
    for kept, p0, p1 in replay(vs, cap, refreshes):
        draws = p1 - p0
        d = {"draws": draws, "kept": len(kept), "filled": bool(draws and len(kept) == cap and vs > cap),
             "before": p0 % STATE, "after": p1 % STATE, "q": None, "row": None, "lane": None, "wave": None,
             "fill_first_round": False, "fill_round_mid_state": False, "fill_at_state_end": False, "end_at_state_end": False,
             "rounds": 0, "states": 0, "mid_state": False, "after_index": None}
        if draws:
            first_state, last_state = p0 // STATE, (p1 - 1) // STATE
            d["rounds"] = d["states"] = last_state - first_state + 1
            d["mid_state"] = p0 % STATE != 0
            d["after_index"] = (p1 - 1) % STATE + 1
            if d["filled"]:
                last = p1 - 1                                   # stream position of the filling draw
                start = max(p0, last // STATE * STATE)          # ... and of the first word of its round
                q = last - start
                d.update(q=q, row=q // ROUND_THREADS, lane=q % WAVE, wave=q % ROUND_THREADS // WAVE,
                         fill_first_round=start == p0, fill_round_mid_state=start == p0 and p0 % STATE != 0,
                         fill_at_state_end=p1 % STATE == 0)
            else:
                d["end_at_state_end"] = p1 % STATE == 0
        out.append(d)
    return out


# ---- the classes of tests/test_gpu_reservoir.py: name -> predicate over one refresh's dict --------------------------------------
CLASSES = {
    "fill_at_state_end": lambda c: c["fill_at_state_end"],
    "end_at_state_end": lambda c: c["end_at_state_end"],
    "fill_q0": lambda c: c["filled"] and c["q"] == 0,
    "fill_row0": lambda c: c["filled"] and c["row"] == 0 and c["q"] > 0,
    "fill_row1": lambda c: c["filled"] and c["row"] == 1,
    "fill_row2": lambda c: c["filled"] and c["row"] == 2,
    "fill_lane0": lambda c: c["filled"] and c["lane"] == 0 and c["q"] > 0,
    "fill_lane63": lambda c: c["filled"] and c["lane"] == 63,
    "fill_first_round": lambda c: c["filled"] and c["fill_first_round"],
    "fill_later_round": lambda c: c["filled"] and not c["fill_first_round"],
    "no_fill_several_states": lambda c: c["draws"] > 0 and not c["filled"] and c["states"] >= 3 and not c["end_at_state_end"],
    "draws_623": lambda c: c["draws"] == 623,
    "draws_624": lambda c: c["draws"] == 624,
    "draws_625": lambda c: c["draws"] == 625,
    "no_draw": lambda c: c["draws"] == 0,
}


def class_test(name):
    """The predicate of a class; `name+mid` asks in addition that the refresh starts in the middle of a state, so that its
    first round has fewer than 624 words."""
    base, _, mid = name.partition("+")
    assert mid in ("", "mid")
    return (lambda c: bool(CLASSES[base](c) and c["mid_state"])) if mid else (lambda c: bool(CLASSES[base](c)))


def in_class(name, vs, cap, refresh):
    return class_test(name)(classify(vs, cap, refresh + 1)[refresh])


def search(cap, name, sizes, refreshes):
    """Smallest vs of `sizes`, and the first refresh below `refreshes`, at which class `name` occurs: (vs, refresh) or None."""
    test = class_test(name)
    for vs in sizes:
        for r, c in enumerate(classify(vs, cap, refreshes)):
            if test(c):
                return vs, r
    return None


# ---- a draw on the threshold ----------------------------------------------------------------------------------------------------
def _convergents(x, q_max):
    """Convergents p/q of the rational x with q <= q_max."""
    p0, q0, p1, q1 = 0, 1, 1, 0
    while True:
        a = x.numerator // x.denominator
        p0, q0, p1, q1 = p1, q1, a * p1 + p0, a * q1 + q0
        if q1 > q_max:
            return
        yield p1, q1
        x -= a
        if x == 0:
            return
        x = 1 / x


def threshold_relation(k, vs, cap):
    """How draw k of the stream stands to the threshold of (vs, cap), in units in the last place of the draw: 0 a tie (kept),
    +1 one ulp above (dropped), -1 one ulp below (kept), None otherwise -- or when refresh 0 never consumes draw k."""
    if vs <= cap or k >= replay(vs, cap, 1)[0][2]:
        return None
    u = uniform(stream(k + 1)[k])
    t = threshold(cap, vs)
    for rel, v in ((0, u), (1, np.nextafter(u, np.float32(-1))), (-1, np.nextafter(u, np.float32(2)))):
        if t == v:
            return rel
    return None


def threshold_designs(relation, k_max=3000, vs_max=20000, limit=None):
    """(k, cap, vs) with threshold_relation(k, vs, cap) == relation, from the convergents of the wanted threshold."""
    found = []
    for k in range(k_max):
        u = uniform(stream(k + 1)[k])
        t = {0: u, 1: np.nextafter(u, np.float32(-1)), -1: np.nextafter(u, np.float32(2))}[relation]
        if not 0 < t < 1:
            continue
        for cap, vs in _convergents(Fraction(float(t)), vs_max):
            if 1 <= cap < vs and threshold(cap, vs) == t and threshold_relation(k, vs, cap) == relation:
                found.append((k, cap, vs))
        if limit and len(found) >= limit:
            break
    return found


# ---- end points -----------------------------------------------------------------------------------------------------------------
def end_points(pairs, image, ords):
    """(own point, partner point), global indices, of the half-links of `image` with these ordinals: the half-links of an image
    are numbered point by point, every point's in the order of the pairs file (Pairs.row_ptr / link_image / link_point)."""
    po = np.asarray(pairs.point_offset, np.int64)
    row = np.asarray(pairs.row_ptr, np.int64)
    l = row[po[image]] + np.asarray(ords, np.int64)
    assert len(l) == 0 or l.max() < row[po[image + 1]]
    own = np.searchsorted(row[po[image]:po[image + 1] + 1], l, side="right") - 1 + po[image]
    partner = po[pairs.link_image[l].astype(np.int64)] + pairs.link_point[l].astype(np.int64)
    return own, partner


def distances(xyz2, own, partner):
    """f32 distance of the end points; exact for integer coordinates whose squared distance is below 2^24, whatever the
    order and contraction of the sum, and sqrt is correctly rounded on every side."""
    d = np.asarray(xyz2, np.float32)[own] - np.asarray(xyz2, np.float32)[partner]
    return np.sqrt((d * d).sum(axis=1, dtype=np.float32))


def virtual_sizes(pairs):
    po = np.asarray(pairs.point_offset, np.int64)
    row = np.asarray(pairs.row_ptr, np.int64)
    return (row[po[1:]] - row[po[:-1]]).astype(np.int64)


# ---- groups whose images have designed numbers of half-links --------------------------------------------------------------------
POINTS = 300
UNLINKED = (0, 1, 2, 150, 151, 298, 299)        # points without any link: start, middle and end of every image


def integer_coordinates(n_points, seed):
    """Integer coordinates below 1000: every squared distance is an integer below 2^22, exact in f32.  Two points in three lie in
    one corner of 20 units, so that the distances of random links are a mixture of a narrow and a wide component, as the fit expects."""
    rng = np.random.default_rng(seed)
    near = rng.random(n_points) < 2 / 3
    return np.where(near[:, None], rng.integers(0, 20, size=(n_points, 3)), rng.integers(0, 1000, size=(n_points, 3))).astype(np.float32)


def _block(rng, n):
    linked = np.setdiff1d(np.arange(POINTS), UNLINKED)
    p1, p2 = rng.choice(linked, n), rng.choice(linked, n)
    d = min(5, n)
    p1[:d], p2[:d] = p1[0], p2[0]               # the first pair of the block up to five times: duplicate links
    return p1.astype(np.uint32), p2.astype(np.uint32)


def hub_group(sizes, seed=1):
    """Image 0 (the hub) paired with image i = 1 .. len(sizes) by sizes[i - 1] pairs: image i has exactly sizes[i - 1]
    half-links, the hub their sum.  Even images stand first in their block and odd ones second; the pairs of image 1 are
    split over two blocks, the second one at the end of the file."""
    from frog_amd.pairs import Pairs
    rng = np.random.default_rng(seed)
    n = len(sizes) + 1
    po = np.arange(n + 1) * POINTS
    blocks, tail = [], None
    for i, vs in enumerate(sizes, start=1):
        p_hub, p_img = _block(rng, vs)
        parts = [(p_hub, p_img)]
        if i == 1 and vs >= 2:
            parts = [(p_hub[:vs // 2], p_img[:vs // 2]), (p_hub[vs // 2:], p_img[vs // 2:])]
        made = [(i, 0, b, a) if i % 2 == 0 else (0, i, a, b) for a, b in parts]
        blocks.append(made[0])
        if len(made) > 1:
            tail = made[1]
    if tail is not None:
        blocks.append(tail)
    return Pairs.from_arrays(po, integer_coordinates(n * POINTS, seed), blocks)


def cycle_group(n_images, block_sizes, seed=1):
    """Images in a cycle, image i paired with image i + 1 by block_sizes[i % len(block_sizes)] pairs: image i has the pairs of
    blocks i - 1 and i as half-links."""
    from frog_amd.pairs import Pairs
    rng = np.random.default_rng(seed)
    po = np.arange(n_images + 1) * POINTS
    blocks = [(i, (i + 1) % n_images, *_block(rng, block_sizes[i % len(block_sizes)])) for i in range(n_images)]
    return Pairs.from_arrays(po, integer_coordinates(n_images * POINTS, seed), blocks)
