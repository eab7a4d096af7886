"""A context's FROG_* switches are its own: read when frog_create is called (frog_amd/csrc/device/switches.h), neither heard
again during the context's life nor fixed for the process by whichever context came first."""
import numpy as np
import pytest

from frog_amd import schedule
from gpu_util import Side

pytestmark = pytest.mark.gpu

TRACED = {"FROG_SETUP_TRACE": "1", "FROG_K11_POINTWISE": "1"}


def _context(pairs, monkeypatch, **env):
    """A context created while the environment holds `env`; the variables are gone before it takes its first step."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s = Side(pairs)
    for k in env:
        monkeypatch.delenv(k)
    return s


def _drive(s, capfd):
    """4 linear iterations, 2 levels of 3 deformable ones: what the run printed to stderr, and everything it computed."""
    capfd.readouterr()
    energies = []

    def on(tag, sides, e=None, infos=None):
        if e is not None:
            energies.append(float(e[0]))
    grids = schedule.run([s], 4, [3, 3], on=on)
    err = capfd.readouterr().err
    lattices = [np.stack([s.grid(i, k)[1] for i in range(s.pairs.n_images)]) for k in range(s.num_grids())]
    return err, (grids, energies, s.xyz(), s.xyz2(), lattices)


def _same(a, b):
    assert a[0] == b[0] and a[1] == b[1] and len(a[1]) >= 4 + 2 * 3
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert len(a[4]) == len(b[4]) >= 2
    for x, y in zip(a[4], b[4]):
        assert np.array_equal(x, y)


def test_a_contexts_switches_are_its_own(small_pairs, monkeypatch, capfd):
    """Context A is created with FROG_SETUP_TRACE=1 and FROG_K11_POINTWISE=1, context B after both are deleted; then both run.
    A's lattice set-ups trace although the variables are gone, B's do not although A was the first context of the process --
    and the same the other way round, the plain context first.  The trace and the transform's form change no bit."""
    for k in TRACED:
        monkeypatch.delenv(k, raising=False)
    results = []
    for traced_first in (True, False):
        first = _context(small_pairs, monkeypatch, **(TRACED if traced_first else {}))
        second = _context(small_pairs, monkeypatch, **({} if traced_first else TRACED))
        err_first, r_first = _drive(first, capfd)
        err_second, r_second = _drive(second, capfd)
        err_traced, err_plain = (err_first, err_second) if traced_first else (err_second, err_first)
        assert err_traced.count("[setup level") >= 2 and err_traced.count("[lattice_alloc]") >= 2, err_traced[-2000:]
        assert "[setup level" not in err_plain and "[lattice_alloc]" not in err_plain, err_plain[-2000:]
        results += [r_first, r_second]
        del first, second
    for r in results[1:]:
        _same(results[0], r)
