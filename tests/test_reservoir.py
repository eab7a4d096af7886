"""The reservoir's NumPy restatement (tests/reservoir_restate.py) against what the project already holds true -- the golden
fixture, SURVEY.md appendix F, the oracle's Stats and, where it is built, the reference's own -- and the designed inputs of
tests/test_gpu_reservoir.py, each asserted to belong to the class it is there for."""
import json
import os

import numpy as np
import pytest

import reservoir_restate as R
from oracle.oracle_api import Stats, ref_lib

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "stats_golden.json")))
CASES = {c["name"]: c for c in GOLDEN["cases"]}

# ---- design constants: found with reservoir_restate.search / threshold_designs, pinned here ------------------------------------
REFRESHES = 7           # every designed event lies at refresh 5 or before: at least one refresh beyond it
# capacity -> [(vs, refresh, class)]; class names are reservoir_restate.CLASSES', `+mid`: the refresh starts in mid-state
DESIGNS = {
    1000: [(1878, 0, "fill_at_state_end"), (1632, 4, "fill_at_state_end+mid"),
           (999, 0, "no_draw"), (1000, 0, "no_draw"), (623, 0, "no_draw"), (624, 0, "no_draw"), (625, 0, "no_draw"),
           (1248, 0, "end_at_state_end"), (1248, 1, "end_at_state_end"), (1248, 2, "end_at_state_end"), (1040, 2, "end_at_state_end+mid"),
           (1881, 0, "fill_q0"), (1570, 5, "fill_q0+mid"), (1022, 5, "fill_row2+mid"), (1001, 4, "fill_row0+mid"),
           (1001, 2, "fill_row1+mid"), (1001, 0, "fill_later_round"), (1011, 0, "fill_lane0"), (1019, 3, "fill_lane0+mid"),
           (1010, 0, "fill_lane63"), (1013, 5, "fill_lane63+mid"),
           (1001, 1, "no_fill_several_states+mid"), (2600, 1, "no_fill_several_states+mid")],
    256: [(631, 2, "fill_at_state_end+mid"), (508, 4, "fill_at_state_end+mid"), (255, 0, "no_draw"), (256, 0, "no_draw"),
          (624, 0, "end_at_state_end"), (312, 1, "end_at_state_end+mid"),
          (476, 3, "fill_q0+mid"), (257, 2, "fill_row0+mid"), (257, 1, "fill_row1+mid"), (577, 1, "fill_row2+mid"),
          (257, 1, "fill_lane0+mid"), (257, 3, "fill_lane63+mid"), (257, 0, "fill_first_round"), (257, 1, "fill_first_round+mid"),
          (257, 2, "fill_later_round+mid"), (634, 5, "no_fill_several_states+mid"),
          (623, 0, "draws_623"), (623, 4, "draws_623+mid"), (624, 0, "draws_624"), (624, 4, "draws_624+mid"),
          (625, 0, "draws_625"), (625, 4, "draws_625+mid")],
    623: [(624, 0, "fill_at_state_end"), (624, 1, "fill_at_state_end"), (622, 0, "no_draw"), (623, 0, "no_draw"),
          (782, 3, "end_at_state_end+mid"),
          (625, 2, "fill_q0+mid"), (625, 5, "fill_row0+mid"), (668, 5, "fill_row1+mid"), (624, 3, "fill_row2+mid"),
          (778, 2, "fill_lane0+mid"), (690, 2, "fill_lane63+mid"), (749, 4, "no_fill_several_states+mid"),
          (624, 3, "fill_later_round+mid"), (624, 2, "draws_623"), (624, 0, "draws_624"), (625, 1, "draws_625")],
}
# classes every capacity's group must reach (a capacity of 1000 cannot fill in a round of 624, nor draw 624 words and stop)
EVERYWHERE = ["fill_at_state_end", "end_at_state_end", "fill_q0", "fill_row0", "fill_row1", "fill_row2", "fill_lane0", "fill_lane63",
              "fill_later_round", "no_fill_several_states", "no_draw"]


def group_sizes(cap):
    """The images of the capacity's group, in the order of their first design."""
    return list(dict.fromkeys(vs for vs, _, _ in DESIGNS[cap]))


# (draw k of the stream, capacity, vs): float32(cap) / float32(vs) against the draw, in refresh 0
TIES = [(436, 423, 719), (488, 557, 777), (571, 622, 797), (540, 999, 1022), (411, 935, 1257), (828, 301, 1361),
        (0, 3446, 6279), (3, 1995, 2363)]
ULP_ABOVE = [(402, 438, 629), (801, 547, 1020), (821, 569, 1109), (943, 239, 1186), (1238, 1384, 1385), (35, 1117, 1167), (17, 349, 1280)]
ULP_BELOW = [(169, 295, 341), (137, 289, 429), (4, 349, 579), (16, 663, 688)]
THRESHOLD_DESIGNS = [(0, d) for d in TIES] + [(1, d) for d in ULP_ABOVE] + [(-1, d) for d in ULP_BELOW]

# the two rings (tests/test_gpu_reservoir.py)
RING80 = {"cap": 64, "sizes": [105, 213, 540], "refreshes": 170}
RING8 = {"cap": 10000, "images": 996, "blocks": [5003, 5003, 5021, 5021], "refreshes": 20}


def oracle_ordinals(which, vs, cap, refreshes):
    s = Stats(which, max_size=cap)
    s.add_slots(vs)
    out = []
    for _ in range(refreshes):
        s.reset()
        s.add_samples(np.arange(vs, dtype=np.float32))         # a sample's value is its ordinal (exact below 2^24)
        out.append(s.samples().astype(np.uint32))
    return out


# ---- the restatement against existing truth -------------------------------------------------------------------------------------
def test_first_word_of_the_stream():
    assert int(R.stream(1)[0]) == R.FIRST_WORD == 2357136044


def test_golden_reservoir_case():
    c = CASES["reservoir"]
    got = R.ordinals(c["virtual_size"], c["max_size"], len(c["kept_ordinals"]))
    assert [o.tolist() for o in got] == c["kept_ordinals"]


def test_survey_appendix_f():
    a, b = R.ordinals(25000, 10000, 2)
    assert len(a) == 10000 and a[:5].tolist() == [11, 13, 15, 17, 18] and a[-1] == 24978
    assert b[:5].tolist() == [1, 4, 5, 6, 9]


def sweep():
    rng = np.random.default_rng(11)
    cases = [(int(vs), int(cap)) for vs, cap in zip(rng.integers(1, 6000, 300), rng.integers(1, 3000, 300))]
    return cases + [(cap + d, cap) for cap in (1, 2, 623, 624, 625) for d in (-1, 0, 1, 2) if cap + d > 0]


def test_restatement_against_the_oracle_stats():
    drew = 0
    for vs, cap in sweep():
        want = oracle_ordinals("oracle", vs, cap, 6)
        got = R.ordinals(vs, cap, 6)
        for r in range(6):
            assert np.array_equal(got[r], want[r]), (vs, cap, r)
        drew += vs > cap
    assert drew > 100


@pytest.mark.skipif(ref_lib() is None, reason="oracle/_ref not built (reference tree absent)")
def test_restatement_against_the_reference_stats():
    designed = [(vs, cap) for cap in DESIGNS for vs in group_sizes(cap)] + [(vs, cap) for _, (_, cap, vs) in THRESHOLD_DESIGNS]
    for vs, cap in sweep()[::3] + designed:
        want = oracle_ordinals("ref", vs, cap, 6)
        got = R.ordinals(vs, cap, 6)
        for r in range(6):
            assert np.array_equal(got[r], want[r]), (vs, cap, r)


# ---- the designs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", sorted(DESIGNS))
def test_every_design_belongs_to_its_class(cap):
    for vs, refresh, name in DESIGNS[cap]:
        assert refresh + 1 < REFRESHES
        assert R.in_class(name, vs, cap, refresh), (cap, vs, refresh, name, R.classify(vs, cap, refresh + 1)[refresh])
    names = {n.partition("+")[0] for _, _, n in DESIGNS[cap]}
    assert set(EVERYWHERE) <= names
    mids = {n for _, _, n in DESIGNS[cap] if n.endswith("+mid")}
    # the position of the filling draw: each with a refresh whose first round starts in mid-state
    assert {"fill_q0+mid", "fill_row0+mid", "fill_row1+mid", "fill_row2+mid", "fill_lane0+mid", "fill_lane63+mid"} <= mids
    sizes = group_sizes(cap)
    assert cap + 1 in sizes and cap in sizes and cap - 1 in sizes
    # images that draw stand before and after the images that do not
    quiet = [k for k, vs in enumerate(sizes) if vs <= cap]
    assert 0 < quiet[0] and quiet[-1] < len(sizes) - 1
    for vs in sizes:                                            # the oracle agrees on every designed size
        want = oracle_ordinals("oracle", vs, cap, REFRESHES)
        got = R.ordinals(vs, cap, REFRESHES)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), (cap, vs)


def test_the_issue_examples_classify_as_stated():
    assert R.classify(1878, 1000, 1)[0]["after_index"] == 624 and R.in_class("fill_at_state_end", 1878, 1000, 0)
    assert R.in_class("fill_at_state_end", 631, 256, 2) and R.in_class("fill_at_state_end", 508, 256, 4)
    assert R.in_class("fill_at_state_end", 624, 623, 0)
    assert all(R.in_class("end_at_state_end", 1248, 1000, r) for r in range(3))
    assert R.in_class("end_at_state_end", 624, 256, 0) and R.in_class("end_at_state_end", 312, 256, 1)
    assert R.classify(1881, 1000, 1)[0]["q"] == 0 and R.classify(1022, 1000, 6)[5]["q"] >= 512
    assert R.classify(1022, 1000, 6)[5]["mid_state"]


def test_search_finds_the_pinned_sizes_again():
    assert R.search(1000, "fill_q0+mid", range(1001, 1600), 6) == (1570, 5)
    assert R.search(256, "fill_at_state_end", range(257, 700), 6) == (508, 4)
    assert R.search(623, "end_at_state_end", range(624, 800), 6) == (782, 3)


@pytest.mark.parametrize("relation,design", THRESHOLD_DESIGNS)
def test_threshold_designs(relation, design):
    k, cap, vs = design
    assert R.threshold_relation(k, vs, cap) == relation
    u, t = R.uniform(R.stream(k + 1)[k]), R.threshold(cap, vs)
    assert {0: u == t, 1: u > t and np.nextafter(t, np.float32(2)) == u, -1: u < t and np.nextafter(u, np.float32(2)) == t}[relation]
    kept = R.ordinals(vs, cap, 1)[0]
    assert (k in kept) == (relation <= 0)                      # the reference tests `random > threshold`: an equal draw is kept
    # they rest on an f32 division: the oracle's Stats says the same, for this refresh and the next
    want = oracle_ordinals("oracle", vs, cap, 2)
    got = R.ordinals(vs, cap, 2)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_threshold_designs_are_enough_of_each_kind():
    assert len(TIES) >= 4 and len(ULP_ABOVE) >= 4 and len(ULP_BELOW) >= 4
    # a threshold formed as cap * (1 / vs) is another number in four designs of the first two kinds, and there the draw changes
    # sides (one ulp below, the product would have to miss the quotient by two ulps: no design below 20 000 half-links does)
    for rel, kind in ((0, TIES), (1, ULP_ABOVE)):
        changed = 0
        for k, cap, vs in kind:
            t2 = np.float32(cap) * (np.float32(1) / np.float32(vs))
            u = R.uniform(R.stream(k + 1)[k])
            changed += bool((u > t2) != (rel > 0))
        assert changed >= 4, rel
    found = R.threshold_designs(0, k_max=100, vs_max=20000)
    assert (0, 3446, 6279) in found and (3, 1995, 2363) in found


def test_ring_designs():
    c = RING80
    classes = [R.classify(vs, c["cap"], c["refreshes"]) for vs in c["sizes"]]
    assert all(x[0]["draws"] > 0 for x in classes)
    # every refresh of 170 draws on every image; fills and misses, and ends of states among them
    assert all(10 < sum(x["filled"] for x in cl) < 160 for cl in classes)
    assert any(x["end_at_state_end"] or x["fill_at_state_end"] for cl in classes for x in cl)
    c = RING8
    b = c["blocks"]
    sizes = sorted({b[(i - 1) % 4] + b[i % 4] for i in range(4)})
    assert len(sizes) == 3 and all(vs > c["cap"] for vs in sizes) and c["images"] % 4 == 0
    # create_statistics: 9 buffers of 12 bytes per kept half-link must exceed 2^30 bytes, 8 must not
    assert 9 * c["images"] * c["cap"] * 12 > 2 ** 30 >= 8 * c["images"] * c["cap"] * 12
    filled = [x["filled"] for vs in sizes for x in R.classify(vs, c["cap"], c["refreshes"])]
    assert any(filled) and not all(filled)


# ---- end points and groups ------------------------------------------------------------------------------------------------------
def test_hub_group_has_the_designed_sizes_and_end_points():
    sizes = [40, 7, 1, 12]
    pairs = R.hub_group(sizes, seed=3)
    assert R.virtual_sizes(pairs).tolist() == [sum(sizes)] + sizes
    po = np.asarray(pairs.point_offset)
    # end points by enumeration: the half-links of an image point by point, each point's in file order
    links = {p: [] for p in range(pairs.n_points)}
    for b in range(pairs.n_blocks):
        i1, i2, p1, p2 = pairs.block(b)
        for a, c in zip(p1, p2):
            links[po[i1] + a].append(po[i2] + c)
            links[po[i2] + c].append(po[i1] + a)
    for image in range(pairs.n_images):
        flat = [(p, q) for p in range(po[image], po[image + 1]) for q in links[p]]
        own, partner = R.end_points(pairs, image, np.arange(len(flat)))
        assert list(zip(own.tolist(), partner.tolist())) == flat
        assert not set(own.tolist()) & {po[image] + u for u in R.UNLINKED}
    assert pairs.n_blocks == len(sizes) + 1                    # image 1's pairs are split over two blocks
    own, partner = R.end_points(pairs, 2, np.arange(7))
    assert len({(a, b) for a, b in zip(own.tolist(), partner.tolist())}) < 7      # duplicate links
    d = R.distances(pairs.xyz, own, partner)
    d2 = ((np.asarray(pairs.xyz, np.int64)[own] - np.asarray(pairs.xyz, np.int64)[partner]) ** 2).sum(axis=1)
    assert d.dtype == np.float32 and np.array_equal(d, np.sqrt(d2.astype(np.float64)).astype(np.float32))


def test_cycle_group_sizes():
    pairs = R.cycle_group(8, [5, 5, 9, 9], seed=2)
    assert R.virtual_sizes(pairs).tolist() == [14, 10, 14, 18, 14, 10, 14, 18]
