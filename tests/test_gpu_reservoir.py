"""The reservoir replay on the device -- k_stats.hip.h select_kernel and sample_resolve_kernel, and the ring of selections
around them in frog_hip.hip (create_statistics, produce_selection, frog_update_stats_local, frog_get_samples) -- on groups whose
images have DESIGNED numbers of half-links, against the NumPy restatement (tests/reservoir_restate.py) and the oracle.

Every refresh sets the same integer coordinates on both sides and compares, per image: the kept ordinals with the restatement;
ordinals, sample distances and (c1, c2, ratio) with OracleGroup, bit for bit; the distances with those of the restatement's own
end points (integer coordinates below 1000: a squared distance is an integer below 2^22, its f32 square root is the same
number however it is summed).  The saved generator state has no getter: every design is followed by at least one more
refresh, whose ordinals a wrong state changes.

The designed sizes, their classes and the threshold designs are pinned in tests/test_reservoir.py, which asserts each
against the classifier on the CPU; here every class is asserted again on the sizes of the group as built.

Left out on purpose: a ring of 2 (the high-priority side stream with one selection ahead: about 30 million kept
half-links); virtualSize clamped at 2^32 - 1; an image without any half-link
(test_gpu_round2.py test_context_that_owns_only_empty_images has it).

Groups: a hub image paired with every designed image by one block, so that image 1 + k has exactly the k-th designed number
of half-links (the hub has their sum, and is compared like the others); 300 points per image, seven of them without a
link at the start, middle and end, duplicate links in every block, one image pair split over two blocks.  The capacity is the
group's, so there is one group per capacity; a threshold design needs a group of its own.
"""
import ctypes as C
import time

import numpy as np
import pytest

import reservoir_restate as R
from frog_amd import _abi
from frog_amd.image_group import ImageGroup
from gpu_util import note
from oracle.oracle_api import OracleGroup
from test_reservoir import DESIGNS, REFRESHES, RING8, RING80, THRESHOLD_DESIGNS, group_sizes

pytestmark = pytest.mark.gpu


def ring_of(g):
    """Buffers in the context's ring of selections: frog_create replays all but one of them ahead."""
    s, n = (C.c_double * 3)(), C.c_int()
    _abi.check(g._lib.frog_create_seconds(g._ctx, s, C.byref(n)), "frog_create_seconds")
    return n.value + 1


def device_ordinals(g, image, cap):
    out, n = np.empty(cap, np.uint32), C.c_int()
    _abi.check(g._lib.frog_get_samples(g._ctx, image, None, out.ctypes.data_as(_abi.c_u32_p), cap, C.byref(n)), "frog_get_samples")
    return out[:n.value]


class Sides:
    """A device context and an oracle over one group, refreshed in step on identical coordinates."""

    def __init__(self, pairs, max_size, image_range=None, oracle=None, **opt):
        self.pairs, self.max_size = pairs, max_size
        self.sizes = R.virtual_sizes(pairs)
        self.g = ImageGroup(pairs, image_range=image_range, stats_max_size=max_size, **opt)
        self.images = range(*image_range) if image_range else range(pairs.n_images)
        self.whole = image_range is None
        if oracle is None:
            oracle = OracleGroup(pairs.model, _abi.FrogOptions.default(stats_max_size=max_size, **opt))
            oracle.setup_stats()
        self.ref = oracle
        self.table = {}
        self.refresh = 0

    def rows(self, image, refreshes):
        """The restatement's refreshes of an image: computed once per size."""
        vs = int(self.sizes[image])
        if vs not in self.table or len(self.table[vs]) < refreshes:
            self.table[vs] = R.replay(vs, self.max_size, refreshes)
        return self.table[vs]

    def coordinates(self, advance_oracle=True):
        x = R.integer_coordinates(self.pairs.n_points, 1000 + self.refresh)
        self.g.set_points2(x)
        if advance_oracle:
            self.ref.set_xyz2(x)
        return x

    def update(self, advance_oracle=True):
        if self.whole:
            self.g.updateStats()
        else:
            _abi.check(self.g._lib.frog_update_stats_local(self.g._ctx), "frog_update_stats_local")
        if advance_oracle:
            self.ref.update_stats()
        self.refresh += 1

    def compare(self, x, total, images=None, oracle=True):
        r = self.refresh - 1
        for i in (self.images if images is None else images):
            want = self.rows(i, total)[r][0]
            s, o = self.g.samples(i)
            assert np.array_equal(o, want), f"ordinals against the restatement: image {i} ({self.sizes[i]} half-links), refresh {r}"
            own, partner = R.end_points(self.pairs, i, want)
            assert np.array_equal(s, R.distances(x, own, partner)), f"end points: image {i}, refresh {r}"
            if oracle:
                rs, ro = self.ref.samples(i)
                assert np.array_equal(o, ro), f"ordinals against the oracle: image {i}, refresh {r}"
                assert np.array_equal(s, rs), f"distances against the oracle: image {i}, refresh {r}"
                assert np.array_equal(self.g.em(i), self.ref.em(i)), f"(c1, c2, ratio): image {i}, refresh {r}"


def designed_group(cap):
    sizes = group_sizes(cap)
    pairs = R.hub_group(sizes, seed=cap)
    assert R.virtual_sizes(pairs).tolist() == [sum(sizes)] + sizes
    return pairs, sizes


@pytest.mark.parametrize("cap,background", [(1000, 0), (1000, 1), (256, 0), (623, 0)])
def test_designed_sizes_at_every_refresh(cap, background):
    pairs, sizes = designed_group(cap)
    both = Sides(pairs, cap, selections_in_background=background)
    assert ring_of(both.g) == 80
    # every class is present in the group as built: image 1 + k has sizes[k] half-links
    built = R.virtual_sizes(pairs)
    for vs, refresh, name in DESIGNS[cap]:
        assert built[1 + sizes.index(vs)] == vs and refresh + 1 < REFRESHES
        assert R.in_class(name, vs, cap, refresh), (cap, vs, refresh, name)
    both.g.setupLinearTransforms(); both.ref.linear_init()
    both.g.transformPoints(); both.ref.transform_points()
    for _ in range(REFRESHES):
        x = both.coordinates()
        both.update()
        both.compare(x, REFRESHES)


@pytest.mark.parametrize("relation,design", THRESHOLD_DESIGNS)
def test_a_draw_on_the_threshold_and_one_ulp_off(relation, design):
    k, cap, vs = design
    assert R.threshold_relation(k, vs, cap) == relation
    pairs = R.hub_group([vs], seed=k)                           # two images of vs half-links each
    both = Sides(pairs, cap)
    both.g.setupLinearTransforms(); both.ref.linear_init()
    both.g.transformPoints(); both.ref.transform_points()
    for refresh in range(2):
        x = both.coordinates()
        both.update()
        both.compare(x, 2)
        if refresh == 0:
            for i in range(2):
                assert (k in both.g.samples(i)[1]) == (relation <= 0)     # `random > threshold` drops: an equal draw is kept


def test_contexts_over_an_image_range():
    """A context's capacity is the largest of min(size, stats_max_size) over ITS images, and image k of the context reads row
    k of its own tables: the same restatement rows and the same oracle as the whole group's."""
    cap = 1000
    pairs, sizes = designed_group(cap)
    quiet = (1 + sizes.index(623), 1 + sizes.index(625) + 1)            # 623, 624, 625: all below the capacity ...
    assert all(vs < cap for vs in sizes[quiet[0] - 1:quiet[1] - 1]) and sizes[0] > cap      # ... an image outside above it
    drawing = (quiet[1], quiet[1] + 6)
    assert all(vs > cap for vs in sizes[drawing[0] - 1:drawing[1] - 1])
    mixed = (quiet[0] - 1, drawing[0] + 2)                              # 1000, the three quiet ones, two that draw
    oracle = OracleGroup(pairs.model, _abi.FrogOptions.default(stats_max_size=cap))
    oracle.setup_stats()
    parts = [Sides(pairs, cap, image_range=rg, oracle=oracle) for rg in (quiet, drawing, mixed)]
    for _ in range(4):
        for n, part in enumerate(parts):
            x = part.coordinates(advance_oracle=n == 0)
            part.update(advance_oracle=n == 0)
            part.compare(x, 4)
    for i in range(*quiet):
        assert len(parts[0].g.samples(i)[1]) == sizes[i - 1]             # every half-link, no draw


def test_ring_of_80_wraps_twice():
    """From refresh 77 on the low-water rule queues one replay per refresh; from the 81st selection on it writes into
    buffers that were consumed."""
    c = RING80
    pairs = R.hub_group(c["sizes"], seed=80)
    t0 = time.perf_counter()
    both = Sides(pairs, c["cap"])
    device = time.perf_counter() - t0
    assert ring_of(both.g) == 80 and c["refreshes"] > 2 * 80
    both.g.setupLinearTransforms(); both.ref.linear_init()
    both.g.transformPoints(); both.ref.transform_points()
    again = None
    for refresh in range(c["refreshes"]):
        t0 = time.perf_counter()
        x = both.coordinates()
        if again is not None:
            # the last refresh's ordinals a second time: its successors' selections have been queued, they are still there
            for i, o in again:
                assert np.array_equal(device_ordinals(both.g, i, c["cap"]), o), (i, refresh)
        both.update()
        both.g.synchronize()
        device += time.perf_counter() - t0
        both.compare(x, c["refreshes"])
        again = [(i, both.rows(i, c["refreshes"])[refresh][0]) for i in range(pairs.n_images)]
    note("reservoir_ring80_seconds", f"{device:.2f} device side (create, {c['refreshes']} x coordinates and refresh) of a 4-image group")


def test_ring_of_8_refills_five_at_a_time():
    """The ring of every large group: more than 2^30 / (12 * 9) kept half-links per context leave at most 8 buffers, refilled
    by five replays in one refresh whenever fewer than three selections are left."""
    c = RING8
    pairs = R.cycle_group(c["images"], c["blocks"], seed=8)
    sizes = R.virtual_sizes(pairs)
    assert len(set(sizes.tolist())) == 3 and sizes.min() > c["cap"]
    opt = dict(stats_max_iterations=2)
    t0 = time.perf_counter()
    both = Sides(pairs, c["cap"], **opt)
    device = time.perf_counter() - t0
    assert ring_of(both.g) == 8
    both.g.setupLinearTransforms(); both.ref.linear_init()
    both.g.transformPoints(); both.ref.transform_points()
    total = c["refreshes"]
    first_images = list(range(8)) + [c["images"] - 1]
    for refresh in range(total):
        t0 = time.perf_counter()
        x = both.coordinates()
        both.update()
        both.g.synchronize()
        got = [device_ordinals(both.g, i, c["cap"]) for i in range(c["images"])]
        device += time.perf_counter() - t0
        for i in range(c["images"]):
            assert np.array_equal(got[i], both.rows(i, total)[refresh][0]), f"image {i} ({sizes[i]} half-links), refresh {refresh}"
        if refresh in (0, 7, total - 1):
            both.compare(x, total)
        # a second time, after the refill's replays have had the time of the comparison above: still the consumed buffer's
        for i in first_images:
            assert np.array_equal(device_ordinals(both.g, i, c["cap"]), got[i]), f"second read: image {i}, refresh {refresh}"
    note("reservoir_ring8_seconds", f"{device:.2f} device side (create, {total} x coordinates, refresh and {c['images']} ordinal reads) "
                                    f"of {c['images']} images, {pairs.n_pairs} pairs")
