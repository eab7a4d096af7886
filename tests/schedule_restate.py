"""The loops of the reference's ImageGroup::run (registration/imageGroup.cxx:54-128) transcribed statement by statement, as a
flat trace of the calls they make: what frog_amd/schedule.py is held to by tests/test_schedule.py.  Deliberately naive, and no
code shared with the driver: the reference's `for` whose rejected iteration does `iteration--; continue` is kept as it is
written (the increment a C `continue` jumps to is the first statement of the loop body here), alpha is the reference's float.

    trace entries   ("init",)  ("stats",)  ("linear",)  ("transform", apply)  ("setup", level)
                    ("deformable", level, bits of the f32 alpha)

`energies` scripts what the steps return, linear ones first, in call order; a negative deformable energy is a rejected step.
The reference has one deformableIterations for all levels; here every level has its own count."""
import numpy as np


def alpha_bits(alpha):
    return int(np.float32(alpha).view(np.uint32))


def run(linear_iterations, deformable_iterations, stat_interval_update, deformable_alpha, energies):
    """-> (trace, grids per level)"""
    trace, energies = [], iter(energies)
    trace.append(("init",))                                                 # :37
    trace.append(("transform", False))                                      # :38
    for iteration in range(linear_iterations):                              # :54
        if not (iteration % stat_interval_update):                          # :59
            trace.append(("stats",))
        trace.append(("linear",)); next(energies)                           # :61
        trace.append(("transform", False))                                  # :63
    trace.append(("transform", True))                                       # :70
    n_grids = []
    for level in range(len(deformable_iterations)):                         # :78
        trace.append(("setup", level))                                      # :81
        trace.append(("transform", False))                                  # :82
        number_of_grids = 1
        alpha = np.float32(deformable_alpha)                                # :84
        number_of_diffeomorphic_iterations = 0
        iteration = -1
        while True:                                                         # :88  for ( iteration = 0; ...; iteration++ )
            iteration += 1
            if not iteration < deformable_iterations[level]:
                break
            if not (iteration % stat_interval_update):                      # :94
                trace.append(("stats",))
            trace.append(("deformable", level, alpha_bits(alpha)))          # :96
            e = next(energies)
            if e < 0:                                                       # :97
                if number_of_diffeomorphic_iterations == 0:                 # :99
                    alpha /= 2                                              # :101
                    alpha = np.float32(alpha)
                number_of_grids += 1                                        # :107
                iteration -= 1                                              # :108
                trace.append(("transform", True))                           # :109
                trace.append(("setup", level))                              # :110
                trace.append(("transform", False))                          # :111
                number_of_diffeomorphic_iterations = 0                      # :112
                continue                                                    # :113
            number_of_diffeomorphic_iterations += 1                         # :117
            trace.append(("transform", False))                              # :118
        n_grids.append(number_of_grids)                                     # :125
        trace.append(("transform", True))                                   # :126
    return trace, n_grids
