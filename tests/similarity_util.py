"""References for the least-squares similarity fit (frog_amd/csrc/device/similarity.h), shared by tests/test_similarity.py and
the RANSAC tests: Horn's closed form at 60 digits with mpmath, Kabsch through numpy's SVD, the error bound both are held to,
and the runner of tests/similarity_driver.cpp."""
import os
import re
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DEVICE = os.path.join(os.path.dirname(HERE), "frog_amd", "csrc", "device")
F4, F8 = np.float32, np.float64
EPS = 2.0 ** -52
# The bound of a fit's entries is K * 2^-52 * magnitude / relgap (see error_bound).  K is four times the worst ratio
# error / (2^-52 * magnitude / relgap) of the numpy SVD solution against the 60-digit one over the accepted cases of
# tests/test_similarity.py, measured 4.7 (the half turn about x; every other case is below 2.3) and taken as 5:
# K = 20.  test_similarity.py::test_svd_reference_is_within_a_quarter_of_K holds the measurement in place.
# similarity_fit itself was not consulted.
K_SVD = 5.0
K = 4.0 * K_SVD


def tau():
    """SIMILARITY_MIN_RELATIVE_GAP as similarity.h states it."""
    text = open(os.path.join(DEVICE, "similarity.h")).read()
    return float.fromhex(re.search(r"SIMILARITY_MIN_RELATIVE_GAP\s*=\s*(0x[0-9a-fp.+-]+)\s*;", text).group(1))


def build_driver(directory, include=DEVICE):
    if not shutil.which("g++"):
        return None
    exe = os.path.join(str(directory), "similarity_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", include,
                    os.path.join(HERE, "similarity_driver.cpp"), "-o", exe], check=True)
    return exe


def run_driver(exe, cases):
    """cases: list of (a, b), float32 (n, 3) each.  Returns (ok bool[m], out float64[m, 4, 4], top2 float64[m, 2])."""
    parts = []
    for a, b in cases:
        ab = np.concatenate([np.asarray(a, F4).reshape(-1, 3), np.asarray(b, F4).reshape(-1, 3)], axis=1)
        parts.append("%d %s\n" % (len(ab), ab.view(np.uint32).astype(">u4").tobytes().hex()))
    r = subprocess.run([exe], input="".join(parts), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr)
    lines = r.stdout.split("\n")
    assert len(lines) == len(cases) + 1 and lines[-1] == ""
    ok = np.zeros(len(cases), bool)
    val = np.zeros((len(cases), 18), F8)
    for i, line in enumerate(lines[:-1]):
        w = line.split()
        assert len(w) == 19
        ok[i] = w[0] == "1"
        val[i] = [float.fromhex(x) for x in w[1:]]
    return ok, val[:, :16].reshape(-1, 4, 4), val[:, 16:]


def horn_matrix_N(M):
    return [[M[0][0] + M[1][1] + M[2][2], M[1][2] - M[2][1], M[2][0] - M[0][2], M[0][1] - M[1][0]],
            [M[1][2] - M[2][1], M[0][0] - M[1][1] - M[2][2], M[0][1] + M[1][0], M[2][0] + M[0][2]],
            [M[2][0] - M[0][2], M[0][1] + M[1][0], -M[0][0] + M[1][1] - M[2][2], M[1][2] + M[2][1]],
            [M[0][1] - M[1][0], M[2][0] + M[0][2], M[1][2] + M[2][1], -M[0][0] - M[1][1] + M[2][2]]]


def horn_mp(a, b, digits=60):
    """Horn's closed form on the float32 inputs as they are, in `digits`-digit arithmetic.  Returns the 4x4 matrix as
    mpmath numbers, the relative gap (l1 - l2) / |l1| of the two largest eigenvalues of N, and the magnitude of the
    entries (see error_bound), the last two as floats."""
    import mpmath as mp
    with mp.workdps(digits):
        n = len(a)
        A = [[mp.mpf(float(v)) for v in p] for p in np.asarray(a, F4)]
        B = [[mp.mpf(float(v)) for v in p] for p in np.asarray(b, F4)]
        ca = [mp.fsum(p[k] for p in A) / n for k in range(3)]
        cb = [mp.fsum(p[k] for p in B) / n for k in range(3)]
        A = [[p[k] - ca[k] for k in range(3)] for p in A]
        B = [[p[k] - cb[k] for k in range(3)] for p in B]
        M = [[mp.fsum(p[r] * q[c] for p, q in zip(A, B)) for c in range(3)] for r in range(3)]
        sa = mp.fsum(v * v for p in A for v in p)
        sb = mp.fsum(v * v for p in B for v in p)
        s = mp.sqrt(sb / sa)
        E, Q = mp.eigsy(mp.matrix(horn_matrix_N(M)))
        order = sorted(range(4), key=lambda k: E[k], reverse=True)
        l1, l2 = E[order[0]], E[order[1]]
        w, x, y, z = (Q[k, order[0]] for k in range(4))
        R = [[w*w + x*x - y*y - z*z, 2 * (x*y - w*z), 2 * (x*z + w*y)],
             [2 * (x*y + w*z), w*w - x*x + y*y - z*z, 2 * (y*z - w*x)],
             [2 * (x*z - w*y), 2 * (y*z + w*x), w*w - x*x - y*y + z*z]]
        out = [[s * R[r][c] for c in range(3)] + [cb[r] - s * mp.fsum(R[r][c] * ca[c] for c in range(3))] for r in range(3)]
        out.append([mp.mpf(0), mp.mpf(0), mp.mpf(0), mp.mpf(1)])
        mag = max([s] + [abs(v) for v in cb] + [s * mp.fsum(abs(v) for v in ca)])
        return out, float((l1 - l2) / abs(l1)), float(mag)


def centred(a, b):
    a, b = np.asarray(a, F4).astype(F8), np.asarray(b, F4).astype(F8)
    ca, cb = a.mean(axis=0), b.mean(axis=0)
    return a - ca, b - cb, ca, cb


def kabsch_svd(a, b):
    """The same least-squares problem through numpy's SVD (Kabsch, determinant corrected to +1, as Umeyama), with Horn's
    symmetric scale sqrt(sum |b'|^2 / sum |a'|^2) and the translation from the centroids.  float64 4x4."""
    a1, b1, ca, cb = centred(a, b)
    U, S, Vt = np.linalg.svd(a1.T @ b1)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    s = np.sqrt((b1 * b1).sum() / (a1 * a1).sum())
    out = np.eye(4)
    out[:3, :3] = s * (Vt.T @ D @ U.T)
    out[:3, 3] = cb - out[:3, :3] @ ca
    return out


def relgap_f64(a, b):
    """(l1 - l2) / |l1| and the magnitude of the entries in float64: for the bound when mpmath is absent."""
    a1, b1, ca, cb = centred(a, b)
    E = np.linalg.eigvalsh(np.array(horn_matrix_N(a1.T @ b1)))
    s = np.sqrt((b1 * b1).sum() / (a1 * a1).sum())
    return float((E[3] - E[2]) / abs(E[3])), float(max(s, np.abs(cb).max(), s * np.abs(ca).sum()))


def error_bound(relgap, mag, k=K):
    """max |entry - reference| allowed: a perturbation of relative size 2^-52 in N turns the dominant eigenvector, and with
    it the rotation, by 2^-52 / relgap; the entries are the rotation times the scale, and the translation is the
    rotation applied to the source centroid: magnitude = max(scale, |target centroid|, scale * |source centroid|_1)."""
    return k * EPS * mag / relgap


def max_error(out, ref_mp):
    """max |out - reference| over the 16 entries, the difference taken in mpmath."""
    import mpmath as mp
    return float(max(abs(mp.mpf(float(out[r][c])) - ref_mp[r][c]) for r in range(4) for c in range(4)))
