"""Makes tests/golden/cli_transcript_*.txt: the stdout of `bin/frog` on the small_pairs group of tests/conftest.py, every
numeric token masked.  The wording is an interface (a UI greps it); test_gpu_cli_and_shards.py compares the build under
test with these files line for line.

    python tests/golden/cli_transcripts.py [path/to/bin/frog]       (needs a GPU)
"""
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
COMMON = ["-li", "12", "-dl", "2", "-di", "10", "-j"]            # no -q: the per-iteration lines are part of it
# -da 2, a step a hundred times the default's, folds the lattice in the first iterations of each level: CANCEL_LINES lines
# "Diffeomorphism is not guaranteed : Iteration canceled" with their halvings and new grids (-da 0.5: 1, -da 1: 4, -da 4: 10)
CANCEL_ALPHA, CANCEL_LINES = "2", 9
RUNS = {"plain": [], "ngl3": ["-ngl", "3"], "cancel": ["-da", CANCEL_ALPHA]}
NUMBER = re.compile(r"[-+]?(?:\d+\.?\d*(?:[eE][-+]?\d+)?|\.\d+(?:[eE][-+]?\d+)?|\bnan\b|\binf\b)")


def mask(text):
    return [NUMBER.sub("#", line) for line in text.splitlines()]


def transcript(frog, pairs, name):
    """Masked stdout lines of one run of `frog` on `pairs` (a frog_amd.pairs.Pairs) in a directory of its own."""
    with tempfile.TemporaryDirectory() as d:
        pairs.write(os.path.join(d, "pairs.bin"))
        r = subprocess.run([frog, "pairs.bin", *COMMON, *RUNS[name]], cwd=d, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return mask(r.stdout)


def golden(name):
    with open(os.path.join(HERE, f"cli_transcript_{name}.txt")) as f:
        return f.read().splitlines()


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from frog_amd.pairs import Pairs
    frog = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "bin", "frog")
    pairs = Pairs.synthetic(6, 3000, 1500, seed=7)
    for name in RUNS:
        lines = transcript(frog, pairs, name)
        assert lines == transcript(frog, pairs, name), f"{name}: two runs print different transcripts"
        with open(os.path.join(HERE, f"cli_transcript_{name}.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
        print(name, len(lines), "lines,", sum("Iteration canceled" in l for l in lines), "cancelled")
