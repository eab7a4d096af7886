"""Lockstep GPU-vs-oracle run printing where the two diverge (diagnostic, not a test)."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from frog_amd import _abi, schedule
from frog_amd.pairs import Pairs
from frog_amd.image_group import ImageGroup
from oracle.oracle_api import OracleGroup

def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30)

pairs = Pairs.synthetic(6, 3000, 1500, seed=7)
g = ImageGroup(pairs); ref = OracleGroup(pairs.model, _abi.FrogOptions.default()); ref.setup_stats()
inject = len(sys.argv) > 1 and sys.argv[1] == "inject"


class Watched:
    """The oracle as a side whose refresh, the second of the two, reports how far the mixtures are apart."""

    def __getattr__(self, name):
        return getattr(ref, name)

    def updateStats(self):
        ref.update_stats()
        d = max(rel(g.em(i), ref.em(i)) for i in range(6))
        same = all(np.array_equal(g.samples(i)[0], ref.samples(i)[0]) for i in range(6))
        print(f"refresh: em rel diff {d:.2e} samples identical {same}")
        if inject:
            for i in range(6): g.set_em(i, ref.em(i))


def on(tag, sides, e=None, infos=None):
    kind = schedule.kind(tag)
    if kind == "linear_done":
        print("after linear: xyz2 rel", rel(g.points()[1], ref.xyz2()))
    elif kind == "step" and e[0] < 0:
        print(f"  regrid at L{tag[1]} it {tag[2]}")
    elif kind == "deformable" and tag[2] % 10 == 9:
        k = g.num_grids() - 1
        d = max(rel(g.grid(i, k)[1], ref.grid(i, k, _abi.FrogGridInfo())[1]) for i in range(6))
        print(f"  L{tag[1]} it {tag[2]}: coeff rel {d:.2e} xyz2 rel {rel(g.points()[1], ref.xyz2()):.2e} E rel {abs(e[0]-e[1])/e[1]:.2e}")


# (this loop used to carry alpha as a Python float: the C ABI takes a float and a halving is exact, so the driver's f32 alpha
# gives the same bits; a guard that decides differently on the two sides now ends the run with the driver's assertion)
schedule.run([g, Watched()], 30, [40] * 3, on=on)
