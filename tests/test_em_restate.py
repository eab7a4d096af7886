"""tests/em_restate.py, the term-by-term restatement of Stats::estimateDistribution, against the oracle's EmStats, the
reference build of stats.cxx (where oracle/_ref is built) and the golden fixture -- bit for bit, from the same start
parameters -- on every case family tests/test_gpu_em_edges.py puts on the device; and the census of every case: the
event a case exists for occurs in it, in the first EM iteration and in the second where the case has one.  That is a
condition on the inputs, checked here so that a later edit of a case cannot quietly empty it."""
import json
import os

import numpy as np
import pytest

import em_restate as er
from oracle.oracle_api import ref_lib

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "stats_golden.json")))
CASES = er.all_cases()


fit, same = er.oracle_fit, er.same


@pytest.fixture(scope="module")
def restated():
    return {c["name"]: er.estimate(c["samples"], c["start"], c["cap"], census_at=(1, 2)) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_restatement_equals_the_oracle(case, restated):
    got, iterations, _ = restated[case["name"]]
    want = fit("oracle", case["samples"], case["start"], case["cap"])
    assert same(got, want), f"{case['name']}: restated {got} oracle {want} after {iterations} iterations"
    if ref_lib() is not None:
        ref = fit("ref", case["samples"], case["start"], case["cap"])
        assert same(got, ref), f"{case['name']}: restated {got} reference build {ref}"


@pytest.mark.parametrize("name", ["em_mixture", "em_warm_start", "em_three_iterations"])
def test_restatement_equals_the_golden_fixture(name):
    c = {k["name"]: k for k in GOLDEN["cases"]}[name]
    got, _, _ = er.estimate(c["samples"], c.get("start_params", er.DEFAULT), c.get("max_iterations", 10000))
    assert np.array_equal(got, np.asarray(c["params"], np.float32)), (got, c["params"])
    want = fit("oracle", c["samples"], c.get("start_params", er.DEFAULT), c.get("max_iterations", 10000))
    assert np.array_equal(got, want)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_each_case_contains_what_it_is_for(case, restated):
    _, iterations, found = restated[case["name"]]
    er.check_wants(case, found, "wants", 1)
    if case["later"]:
        assert iterations >= 2, f"{case['name']}: the fit stopped after {iterations} iteration(s)"
        er.check_wants(case, found, "later", 2)
    if case["start"] == tuple(float(np.float32(a)) for a in er.T0):
        for it in found:
            assert not found[it]["t"].any(), f"{case['name']}: a membership is not 0 in iteration {it}"
    if case["start"] == tuple(float(np.float32(a)) for a in er.T1):
        smp = case["samples"]
        assert np.all(found[1]["t"][smp > 0] == 1), f"{case['name']}: a membership of a non-zero sample is not 1"


def test_the_families_leave_clean_batches_too():
    """(e): batches of 64 with none of the events, which the kernel may take the short way -- the ordinary counts have them in
    every accumulator, so the short way is walked next to every special one."""
    _, _, found = er.estimate(er.two_scale(8193, 108), er.DEFAULT, census_at=(2,))
    for acc in er.ACCUMULATORS:
        c = found[2][acc]
        assert c["clean_batches"] >= 64 and c["clean_batches"] < c["batches"], (acc, c["clean_batches"], c["batches"])


def test_census_on_a_hand_made_chain():
    """2^23 (ulp 1), then 0.5 on an even sum (stays), 1, 0.5 on an odd sum (goes up), 0.5 + 2^-21 (near, up), 2^23 (exit)."""
    v = np.array([2.0 ** 23, 0.5, 1.0, 0.5, 0.5 + 2.0 ** -21, 2.0 ** 23])
    sums = er.chain_f64(v)
    assert list(sums) == [2.0 ** 23, 2.0 ** 23, 2.0 ** 23 + 1, 2.0 ** 23 + 2, 2.0 ** 23 + 3, 2.0 ** 24 + 4]
    c = er.census(sums, v)
    assert (c["special"], c["tie_even"], c["tie_odd"], c["tie_up"], c["tie_down"], c["near"], c["exit"]) == (1, 1, 1, 1, 1, 1, 1)
    assert list(c["exit_at"]) == [5] and c["clean_batches"] == 0
