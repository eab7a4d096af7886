"""The iteration schedule of the reference's ``ImageGroup::run`` (registration/imageGroup.cxx:54-128), stated once
for every Python host and test.

A *side* is anything with the reference's six method names -- ``setupLinearTransforms()``,
``transformPoints(apply=False)``, ``updateStats()``, ``updateLinearTransforms() -> E``,
``setupDeformableTransforms(level) -> info`` and ``updateDeformableTransforms(alpha) -> E``: an ``ImageGroup``, a
``ShardedImageGroup``, a CPU restatement under test.  Several sides run in lockstep, each on its own state: every verb goes to all of
them before the next verb, and they must agree on every decision of the diffeomorphism guard.

``on(tag, sides, e=None, infos=None)``, when given, is called at
  ``"init"``                      after the initial transform,
  ``("linear", it)``              after a linear iteration's transform, with the sides' energies,
  ``"linear_done"``               after the transform that re-bases the points on the linear result (:70),
  ``("setup", level)``            after every lattice set-up and its transform, with the sides' grid infos,
  ``("step", level, it)``         after a deformable step, before the guard's accept / reject branch, with the energies,
  ``("deformable", level, it)``   after an accepted step's transform, with the energies,
  ``("level_done", level)``       after a level's last iteration, before its re-basing transform (where the reference
                                  counts inliers, :123).
"""
import numpy as np


def kind(tag):
    """"linear" of ("linear", it); a bare tag is its own kind."""
    return tag if isinstance(tag, str) else tag[0]


def run_linear(sides, iterations, stat_interval, on=None):
    """:54-66."""
    for it in range(iterations):
        if it % stat_interval == 0:
            for s in sides: s.updateStats()
        e = [s.updateLinearTransforms() for s in sides]
        for s in sides: s.transformPoints()
        if on: on(("linear", it), sides, e)


def run_level(sides, level, iterations, stat_interval, alpha0, on=None):
    """One deformable level, :81-126.  A step with E < 0 was rejected by the guard: alpha is halved (in f32, as the
    reference's float) only if no step was accepted on the current lattice, the points are re-based, a new lattice is
    set up and the SAME iteration index is replayed -- its statistics refresh included.  Returns the lattices made."""
    def setup():
        infos = [s.setupDeformableTransforms(level) for s in sides]
        for s in sides: s.transformPoints()
        if on: on(("setup", level), sides, infos=infos)
    setup()
    alpha, accepted, n_grids, it = np.float32(alpha0), 0, 1, 0
    while it < iterations:
        if it % stat_interval == 0:
            for s in sides: s.updateStats()
        e = [s.updateDeformableTransforms(float(alpha)) for s in sides]
        assert len({x < 0 for x in e}) == 1, f"guard decisions differ at level {level}, iteration {it}: {e}"
        if on: on(("step", level, it), sides, e)
        if e[0] < 0:
            if accepted == 0:
                alpha = np.float32(alpha / np.float32(2))
            n_grids += 1
            for s in sides: s.transformPoints(True)
            setup()
            accepted = 0
            continue
        accepted += 1
        for s in sides: s.transformPoints()
        if on: on(("deformable", level, it), sides, e)
        it += 1
    if on: on(("level_done", level), sides)
    for s in sides: s.transformPoints(True)
    return n_grids


def run(sides, linear_iterations, per_level, stat_interval=10, alpha0=0.02, on=None):
    """The whole schedule; ``per_level`` lists the deformable iterations of each level.  Returns the lattices per level."""
    for s in sides: s.setupLinearTransforms()
    for s in sides: s.transformPoints()
    if on: on("init", sides)
    run_linear(sides, linear_iterations, stat_interval, on)
    for s in sides: s.transformPoints(True)
    if on: on("linear_done", sides)
    return [run_level(sides, level, n, stat_interval, alpha0, on) for level, n in enumerate(per_level)]
