"""frog_amd/schedule.py against the transcription of the reference's loops (tests/schedule_restate.py): the same calls in the
same order, alpha to the bit, on scripted energies -- no device.  And ImageGroup.run's own bookkeeping around the driver."""
import numpy as np
import pytest

import schedule_restate
from frog_amd import schedule
from frog_amd.image_group import ImageGroup


class FakeSide:
    """Records the restatement's trace entries into `trace` (shared by the sides of a run) and answers from a script."""

    def __init__(self, trace, energies):
        self.trace, self.energies, self.level = trace, iter(energies), None

    def setupLinearTransforms(self):
        self.trace.append(("init",))

    def transformPoints(self, apply=False):
        self.trace.append(("transform", bool(apply)))

    def updateStats(self):
        self.trace.append(("stats",))

    def updateLinearTransforms(self):
        self.trace.append(("linear",))
        return next(self.energies)

    def setupDeformableTransforms(self, level):
        self.level = level
        self.trace.append(("setup", level))
        return ("info", level)

    def updateDeformableTransforms(self, alpha):
        assert isinstance(alpha, float)
        self.trace.append(("deformable", self.level, schedule_restate.alpha_bits(alpha)))
        return next(self.energies)


def drive(li, per_level, si, energies, n_sides=1, on=None, alpha0=0.02):
    trace = []
    sides = [FakeSide(trace, energies) for _ in range(n_sides)]
    grids = schedule.run(sides, li, per_level, si, alpha0, on)
    for s in sides:
        assert next(s.energies, None) is None, "the script was not used up"
    return trace, grids


# (linear iterations, iterations per level, energies in call order: linear first; negative = rejected step)
SCRIPTS = {
    "no_rejection": (3, [2, 2], [9, 8, 7, 6, 5, 4, 3]),
    "rejection_at_iteration_0": (2, [3], [9, 8, -1, 5, 4, 3]),
    "two_rejections_in_a_row": (1, [2, 1], [9, -1, -1, 5, 4, 3]),
    "rejection_after_accepted_steps_then_at_the_new_lattices_first": (0, [5], [5, 4, -1, -1, 3, 2, 1]),
    "rejection_at_a_positive_multiple_of_the_interval": (4, [8], [9, 8, 7, 6, 5, 5, 5, -1, 5, 5, 5, -1, -1, 5, 5]),
    "zero_linear_iterations": (0, [2], [5, 4]),
    "a_zero_iteration_level": (2, [2, 0, 1], [9, 8, 5, -1, 4, 3]),
    "different_counts_per_level": (11, [4, 1, 7], [9] * 11 + [5, 4, 3, 2] + [-1, 5] + [5, 5, 5, -1, 5, -1, -1, 5, 5, 5]),
}


@pytest.mark.parametrize("si", [1, 3, 10])
@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_the_driver_makes_the_reference_loops_calls(name, si):
    li, per_level, energies = SCRIPTS[name]
    want = schedule_restate.run(li, per_level, si, 0.02, energies)
    assert drive(li, per_level, si, energies) == want


def alphas(trace):
    return [np.array(t[2], np.uint32).view(np.float32) for t in trace if t[0] == "deformable"]


def test_a_rejection_at_iteration_0_refreshes_twice_and_halves_alpha():
    trace, grids = drive(0, [2], 10, [-1, 5, 4])
    assert trace[3:] == [("setup", 0), ("transform", False),
                         ("stats",), ("deformable", 0, schedule_restate.alpha_bits(0.02)),
                         ("transform", True), ("setup", 0), ("transform", False),
                         ("stats",), ("deformable", 0, schedule_restate.alpha_bits(np.float32(0.02) / np.float32(2))), ("transform", False),
                         ("deformable", 0, schedule_restate.alpha_bits(np.float32(0.02) / np.float32(2))), ("transform", False),
                         ("transform", True)]
    assert grids == [2]


def test_alpha_halves_only_when_no_step_was_accepted_on_the_lattice():
    a = np.float32(0.02)
    h, q = np.float32(a / np.float32(2)), np.float32(a / np.float32(4))
    assert alphas(drive(0, [2], 10, [-1, -1, 5, 4])[0]) == [a, h, q, q]                     # twice in a row: halved twice
    # accepted, accepted, rejected (no halving), rejected at the new lattice's first step (halving), accepted ...
    assert alphas(drive(0, [5], 10, [5, 4, -1, -1, 3, 2, 1])[0]) == [a, a, a, a, h, h, h]
    assert alphas(drive(0, [1, 1], 10, [-1, 5, 4])[0]) == [a, h, a]                          # every level starts from alpha0


def test_a_rejection_at_a_multiple_of_the_interval_repeats_the_refresh():
    trace, _ = drive(0, [5], 3, [5, 5, 5, -1, 5, 5])
    stats_before = [i for i, t in enumerate(trace) if t[0] == "deformable" and trace[i - 1] == ("stats",)]
    steps = [i for i, t in enumerate(trace) if t[0] == "deformable"]
    assert stats_before == [steps[0], steps[3], steps[4]]           # iteration 0, iteration 3 rejected, iteration 3 replayed


@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_two_sides_in_lockstep_get_every_verb_before_the_next_verb(name):
    li, per_level, energies = SCRIPTS[name]
    want, want_grids = schedule_restate.run(li, per_level, 3, 0.02, energies)
    trace, grids = drive(li, per_level, 3, energies, n_sides=2)
    assert trace == [t for t in want for _ in range(2)] and grids == want_grids


def test_sides_that_disagree_on_a_guard_decision_stop_the_run():
    trace = []
    a = FakeSide(trace, [9, 5, 4, 3, 5, 4, 3])
    b = FakeSide(trace, [9, 5, 4, 3, 5, -1, 3])
    with pytest.raises(AssertionError, match=r"level 1, iteration 1\b"):
        schedule.run([a, b], 1, [3, 3], 10, 0.02)


def test_hook_tags_and_where_they_arrive():
    trace = []
    sides = [FakeSide(trace, [9, 8, -1, 5, 4])]
    seen = []

    def on(tag, got_sides, e=None, infos=None):
        assert got_sides is sides
        trace.append(("hook", tag))
        seen.append((tag, e, infos))
    schedule.run(sides, 2, [1, 1, 0], 10, 0.02, on)
    assert [t for t, _, _ in seen] == ["init", ("linear", 0), ("linear", 1), "linear_done",
                                       ("setup", 0), ("step", 0, 0), ("setup", 0), ("step", 0, 0), ("deformable", 0, 0), ("level_done", 0),
                                       ("setup", 1), ("step", 1, 0), ("deformable", 1, 0), ("level_done", 1),
                                       ("setup", 2), ("level_done", 2)]
    assert [e for _, e, _ in seen if e is not None] == [[9], [8], [-1], [5], [5], [4], [4]]
    assert [i for _, _, i in seen if i is not None] == [[("info", 0)], [("info", 0)], [("info", 1)], [("info", 2)]]
    at = trace.index
    assert trace[at(("hook", "init")) - 2:at(("hook", "init"))] == [("init",), ("transform", False)]
    i = at(("hook", "linear_done"))                                  # after the re-basing transform, before the first set-up
    assert trace[i - 1] == ("transform", True) and trace[i - 2] == ("hook", ("linear", 1)) and trace[i + 1] == ("setup", 0)
    i = at(("hook", ("step", 0, 0)))                                  # after the step, before the reject branch's re-basing
    assert trace[i - 1][0] == "deformable" and trace[i + 1] == ("transform", True)
    i = at(("hook", ("deformable", 0, 0)))                            # after the accepted step's transform
    assert trace[i - 2] == ("hook", ("step", 0, 0)) and trace[i - 1] == ("transform", False)
    for level in range(3):                                            # after the level's last iteration, before its re-basing
        i = at(("hook", ("level_done", level)))
        assert trace[i + 1] == ("transform", True) and trace[i - 1][0] == "hook"
    assert trace[-1] == ("transform", True)
    assert schedule.kind("init") == "init" and schedule.kind(("step", 1, 2)) == "step"


# ---- ImageGroup.run around the driver, without a context ---------------------------------------------------------------------

def scripted_group(energies, **attrs):
    """An ImageGroup without a context whose six verbs are a FakeSide's."""
    g = ImageGroup.__new__(ImageGroup)
    g.__dict__.update(dict(linearIterations=2, deformableLevels=2, deformableIterations=2, deformableAlpha=0.02,
                           statIntervalUpdate=10, measures=["stale"], gridsPerLevel=["stale"], _ctx=None, calls=[]), **attrs)
    fake = FakeSide(g.calls, energies)
    for verb in ("setupLinearTransforms", "transformPoints", "updateStats", "updateLinearTransforms",
                 "setupDeformableTransforms", "updateDeformableTransforms"):
        setattr(g, verb, getattr(fake, verb))
    return g


def test_image_group_run_measures_log_and_grids_per_level():
    energies = [0.1, 1.0 / 3.0, 2.5, -1.0, 1e-3, 7.0, 6.0]
    g = scripted_group(energies)
    lines = []
    measures = g.run(log=lines.append)
    accepted = [e for e in energies if e >= 0]
    want = [float(np.float32(e)) for e in accepted]
    assert measures is g.measures and measures == want and measures != accepted          # rounded to f32, as the reference's float
    assert lines == ["Linear registration"] + [f"E = {e:g}" for e in want]
    assert g.gridsPerLevel == [2, 1]
    assert g.calls == schedule_restate.run(2, [2, 2], 10, 0.02, energies)[0]
    quiet = scripted_group(energies, statIntervalUpdate=1, deformableAlpha=0.5)
    assert quiet.run() == want                                                           # no log: nothing to call
    assert quiet.calls == schedule_restate.run(2, [2, 2], 1, 0.5, energies)[0]


def test_image_group_run_stops_on_a_nan_energy():
    g = scripted_group([0.5, 0.25, 2.0, float("nan"), 1.0])
    lines = []
    with pytest.raises(FloatingPointError, match="NaN"):
        g.run(log=lines.append)
    assert g.measures == [0.5, 0.25, 2.0] and lines[-1] == "E = nan"
