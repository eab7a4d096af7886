"""What the GPU test modules share: the numbers file, the relative error, a group of either kind behind one set of
read-back names, the ragged test group, bin/frog runs and their comparison, and the product path against
reference-order mode (tests/test_gpu_reference_order.py, tests/test_gpu_round6.py).  The schedule itself is
frog_amd.schedule's."""
import csv
import json
import os
import subprocess

import numpy as np

from frog_amd import _abi, schedule
from frog_amd.image_group import ImageGroup
from frog_amd.pairs import Pairs
from oracle.oracle_api import OracleGroup
from lattice_util import lattice_deviation, node_weights, lattice_taps, face_crossing_nodes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# k_links.hip.h INLIER_PROBABILITY_BOUND: the derived bound of the fast inlier weight against the reference's form
INLIER_PROBABILITY_BOUND = 2.0 ** -16


def note(name, value):
    """Numbers DESIGN.md quotes: appended to gpurun_out/test_numbers.txt when that directory exists."""
    d = os.path.join(ROOT, "gpurun_out")
    if os.path.isdir(d):
        with open(os.path.join(d, "test_numbers.txt"), "a") as fh:
            fh.write(f"{name} {value}\n")


def relerr(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


def _run_schedule(pairs, monkeypatch, cull, skin=None, **opt):
    monkeypatch.setenv("FROG_CULL", "1" if cull else "0")
    if skin:
        monkeypatch.setenv("FROG_CULL_SKIN", skin)
    else:
        monkeypatch.delenv("FROG_CULL_SKIN", raising=False)
    g = ImageGroup(pairs, **opt)
    g.linearIterations, g.deformableLevels, g.deformableIterations = 20, 3, 25
    E = g.run()
    lattices = [[g.grid(i, k)[1].copy() for k in range(g.num_grids())] for i in range(pairs.n_images)]
    sums = g.point_sums().copy()
    counts = [(c.inliers, c.outliers) for c in g.countInliers()]
    return g, E, lattices, sums, counts, g.points()[1].copy()


class Side:
    """The HIP path (ImageGroup) or the oracle (OracleGroup) as a side of frog_amd.schedule: the six verbs, and every other
    name the two groups share, are the group's own; the read-back accessors whose names or signatures differ are here."""

    def __init__(self, pairs, oracle=False, **opt):
        self.oracle = oracle
        self.pairs = pairs
        self.first = int(opt.get("n_fixed_images", 0))       # -fi: the first images are fixed, the context owns the others
        if oracle:
            self.g = OracleGroup(pairs.model, _abi.FrogOptions.default(**opt))
            self.g.setup_stats()
            self.g.keep_raw_gradient(True)
        else:
            self.g = ImageGroup(pairs, **opt)

    def __getattr__(self, name):
        if name == "g":                 # (a constructor that raised left no group behind)
            raise AttributeError(name)
        return getattr(self.g, name)

    def xyz(self):
        return self.g.xyz() if self.oracle else self.g.points()[0]

    def xyz2(self):
        return self.g.xyz2() if self.oracle else self.g.points()[1]

    def matrices(self):
        return np.stack([self.g.matrix(i) for i in range(self.first, self.pairs.n_images)])

    def ems(self):
        return np.stack([self.g.em(i) for i in range(self.pairs.n_images)])

    def gradient_raw(self, image, n_cp):
        return self.g.gradient_raw(image, n_cp) if self.oracle else self.g.gradient(image, n_cp)

    def grid(self, image, k):
        return self.g.grid(image, k, _abi.FrogGridInfo()) if self.oracle else self.g.grid(image, k)


def ragged_pairs(seed=5):
    """Images of 25 .. 1500 points observing subsets of one landmark cloud: true matches between
    co-observed landmarks, 25 % false matches, points without any link, one image pair with heavy
    duplication (400 links of ONE point into the same partner image) and one image pair whose
    block appears twice in the file."""
    rng = np.random.default_rng(seed)
    sizes = [1500, 25, 700, 40, 1100, 260]
    po = np.concatenate([[0], np.cumsum(sizes)])
    cloud = rng.uniform(0, 300, size=(1500, 3))
    seen = [rng.permutation(1500)[:n] for n in sizes]            # landmark of every point
    xyz = np.concatenate([(cloud[seen[i]] * rng.uniform(0.9, 1.1, 3) + rng.uniform(-30, 30, 3)
                           + rng.normal(0, 1.5, (sizes[i], 3))).astype(np.float32) for i in range(len(sizes))])
    where = []
    for i in range(len(sizes)):
        w = -np.ones(1500, np.int64); w[seen[i]] = np.arange(sizes[i]); where.append(w)
    blocks = []
    for i in range(len(sizes)):
        for j in range(i + 1, len(sizes)):
            both = np.nonzero((where[i] >= 0) & (where[j] >= 0))[0]
            both = both[rng.random(len(both)) < 0.8]             # some co-observed landmarks stay unlinked
            p1, p2 = where[i][both], where[j][both]
            nf = max(2, len(both) // 3)
            p1 = np.concatenate([p1, rng.integers(0, sizes[i], nf)])
            p2 = np.concatenate([p2, rng.integers(0, sizes[j], nf)])
            if (i, j) == (0, 2):
                p1 = np.concatenate([p1, np.full(400, 7)])       # 400 links of point 7 of image 0 into image 2
                p2 = np.concatenate([p2, rng.integers(0, 20, 400)])
            order = np.argsort(p1, kind="stable")
            blocks.append((i, j, p1[order].astype(np.uint32), p2[order].astype(np.uint32)))
    blocks.append(blocks[1])                                     # the same image pair appears twice in the file
    return Pairs.from_arrays(po, xyz, blocks)


# ---- bin/frog on a directory that holds pairs.bin, and two such runs compared ---------------------------------------------------

def _frog(cwd, *flags, env_extra=None):
    env = dict(os.environ)
    env.pop("FROG_THREE_COLLECTIVES", None)
    env.update(env_extra or {})
    r = subprocess.run([os.path.join(ROOT, "bin", "frog"), "pairs.bin", "-li", "12", "-dl", "2", "-di", "10", "-j", "-q", "1", *flags],
                       cwd=cwd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _same_files(a, b, n_images):
    """measures.csv and every transforms/<i>.json: the same text."""
    assert open(a / "measures.csv").read() == open(b / "measures.csv").read()
    for i in range(n_images):
        assert open(a / "transforms" / f"{i}.json").read() == open(b / "transforms" / f"{i}.json").read(), i


def _compare_runs(a, b, n_images, tol=1e-6):
    ea = np.array([float(x[1]) for x in list(csv.reader(open(a / "measures.csv")))[1:]])
    eb = np.array([float(x[1]) for x in list(csv.reader(open(b / "measures.csv")))[1:]])
    assert len(ea) == len(eb) and np.max(np.abs(ea - eb) / eb) < 1e-5       # six printed digits
    for i in range(n_images):
        ta = json.load(open(a / "transforms" / f"{i}.json"))["transforms"]
        tb = json.load(open(b / "transforms" / f"{i}.json"))["transforms"]
        assert len(ta) == len(tb)
        assert relerr(ta[0]["matrix"], tb[0]["matrix"]) < tol
        for x, y in zip(ta[1:], tb[1:]):
            assert x["dimensions"] == y["dimensions"] and relerr(x["coeffs"], y["coeffs"]) < 10 * tol
    ba, bb = json.load(open(a / "bbox.json")), json.load(open(b / "bbox.json"))
    assert ba["halfPairs"] == bb["halfPairs"] and abs(ba["inliers"] - bb["inliers"]) <= 2
    assert relerr(ba["bbox"], bb["bbox"]) < tol
    ha = list(csv.reader(open(a / "histograms.csv"))); hb = list(csv.reader(open(b / "histograms.csv")))
    assert ha[0] == hb[0] and len(ha) == len(hb)


# ---- the product path against reference-order mode, both on the device --------------------------------------------------

def dense_field_deviation(a, b, k, images, xyz, n_per_axis=24, skip=None):
    """Displacement of lattice k on both sides on a dense lattice of points over the bounding box of the coordinates the
    lattice acts on (what a resampler evaluates: tools/VolumeTransform.cxx:119-136), relative to the largest displacement.
    skip: mask of control points whose difference is left out (tests/lattice_util.py face_crossing_nodes)."""
    lo, hi = xyz.min(axis=0).astype(np.float64), xyz.max(axis=0).astype(np.float64)
    axes = [np.linspace(lo[d], hi[d], n_per_axis) for d in range(3)]
    pts = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)
    worst, scale = 0.0, 0.0
    for i in images:
        info, ca = a.grid(i, k)
        _, cb = b.grid(i, k)
        idx, wt = lattice_taps(pts, info)
        diff = ca.astype(np.float64) - cb
        if skip is not None:
            diff[skip] = 0.0
        db = np.einsum("nt,ntk->nk", wt, cb.astype(np.float64)[idx])
        worst = max(worst, float(np.max(np.abs(np.einsum("nt,ntk->nk", wt, diff[idx])))))
        scale = max(scale, float(np.max(np.abs(db))))
    return worst / max(scale, 1e-30), scale


class RefAsOracle:
    """Adapter: a reference-order device side seen through the oracle's getter names (for tests/lattice_util.py)."""

    def __init__(self, side):
        self.s = side
        self.n_images = side.pairs.n_images

    def grid(self, image, k, info=None):
        return self.s.g.grid(image, k)


def fast_against_reference_order(pairs, li, dl, di, monkeypatch, images, **opt):
    monkeypatch.setenv("FROG_REFERENCE_ORDER", "1")
    ref = Side(pairs, **opt)
    monkeypatch.delenv("FROG_REFERENCE_ORDER")
    fast = Side(pairs, **opt)
    po = np.asarray(pairs.point_offset)
    snaps, snaps_fast, worst = [], [], {"E": 0.0}

    def check(tag, sides, e=None, infos=None):
        if infos is not None:
            assert list(infos[0].dims) == list(infos[1].dims), tag
            snaps.append(sides[1].xyz().copy())
            snaps_fast.append(sides[0].xyz().copy())
        if e is not None and e[0] >= 0 and tag[0] != "step":
            worst["E"] = max(worst["E"], abs(e[0] - e[1]) / abs(e[1]))
    grids = schedule.run([fast, ref], li, [di] * dl, on=check)
    out = []
    adapter = RefAsOracle(ref)
    for k in range(ref.num_grids()):
        w = node_weights(adapter, k, po, snaps[k])
        d = {"raw": 0.0, "weighted": 0.0, "field": 0.0}
        for i in images:
            r = lattice_deviation(fast.g, adapter, k, i, snaps[k][po[i]:po[i + 1]], w)
            if r["raw"] >= d["raw"]:
                d["raw_image"] = int(i)
                for key in ("raw_node", "raw_node_weight", "raw_node_support", "raw_node_points"):
                    d[key] = r[key]
            for key in ("raw", "weighted", "field"):
                d[key] = max(d[key], r[key])
            d["weak"], d["nodes"] = r["weak"], r["nodes"]
        d["dense_field"], d["max_disp"] = dense_field_deviation(fast.g, ref.g, k, images, snaps[k])
        # control points one of the two runs reaches across a cell face (tests/lattice_util.py): counted, and the same two
        # numbers without them
        info = ref.g.grid(0 + ref.first, k)[0]
        crossing, skip = face_crossing_nodes(snaps_fast[k], snaps[k], info)
        d["face_crossings"], d["crossing_nodes"] = int(len(crossing)), int(skip.sum())
        d["raw_elsewhere"], d["dense_field_elsewhere"] = d["raw"], d["dense_field"]
        if len(crossing):
            d["raw_elsewhere"], scale = 0.0, 0.0
            for i in images:
                ca, cb = fast.g.grid(i, k)[1], ref.g.grid(i, k)[1]
                d["raw_elsewhere"] = max(d["raw_elsewhere"], float(np.abs(ca.astype(np.float64) - cb)[~skip].max()))
                scale = max(scale, float(np.abs(cb).max()))
            d["raw_elsewhere"] /= max(scale, 1e-30)
            d["dense_field_elsewhere"] = dense_field_deviation(fast.g, ref.g, k, images, snaps[k], skip=skip)[0]
        out.append(d)
    # the WHOLE chain of an image (matrix, then every lattice in creation order: what transforms/<i>.json holds and
    # tools/VolumeTransform.cxx / PointsTransform.cxx evaluate) on a dense lattice of points over the image's own keypoint
    # box, through the device's chain evaluation (include/frog_chain.h): deviation of the displacement T(x) - x
    from frog_amd.chain import Chain, Link
    chain = {"rel": 0.0, "mm": 0.0, "max_disp_mm": 0.0}
    x0 = np.asarray(pairs.xyz, np.float64).reshape(-1, 3)
    for i in images:
        pts_i = x0[po[i]:po[i + 1]]
        lo, hi = pts_i.min(axis=0), pts_i.max(axis=0)
        grid = np.stack(np.meshgrid(*[np.linspace(lo[d], hi[d], 20) for d in range(3)], indexing="ij"), axis=-1).reshape(-1, 3)
        disp = []
        for side in (fast, ref):
            links = [Link.linear(side.g.matrix(i))]
            for k in range(side.num_grids()):
                info, c = side.g.grid(i, k)
                links.append(Link.bspline(list(info.dims), list(info.origin), list(info.spacing), c))
            ch = Chain(links)
            disp.append(ch.apply(grid) - grid)
            ch.close()
        dev = float(np.max(np.abs(disp[0] - disp[1])))
        scale = float(np.max(np.abs(disp[1])))
        chain["mm"] = max(chain["mm"], dev); chain["max_disp_mm"] = max(chain["max_disp_mm"], scale)
        chain["rel"] = max(chain["rel"], dev / max(scale, 1e-30))
    mf, mr = fast.matrices(), ref.matrices()
    diag = lambda a: np.stack([a[:, 0, 0], a[:, 1, 1], a[:, 2, 2]])
    m = max(float(np.max(np.abs(diag(mf) - diag(mr))) / np.max(np.abs(diag(mr)))),
            float(np.max(np.abs(mf[:, :3, 3] - mr[:, :3, 3])) / np.max(np.abs(mr[:, :3, 3]))))
    x = float(np.max(np.abs(fast.xyz().astype(np.float64) - ref.xyz())) / np.max(np.abs(ref.xyz())))
    ca, cb = fast.g.countInliers(), ref.g.countInliers()
    census = sum(abs(ca[i].inliers - cb[i].inliers) for i in range(pairs.n_images))
    return {"lattices": out, "grids": grids, "E": worst["E"], "matrices": m, "xyz": x, "census": census, "chain": chain}


def report(name, r):
    note(name, f"E {r['E']:.2e} matrices {r['matrices']:.2e} xyz {r['xyz']:.2e} grids {r['grids']} census_differs_by {r['census']} "
               f"whole_chain_dense rel {r['chain']['rel']:.2e} abs {r['chain']['mm']:.2e} mm of {r['chain']['max_disp_mm']:.1f} mm")
    for k, d in enumerate(r["lattices"]):
        note(f"{name}_lattice_{k}", " ".join(f"{a} {b:.2e}" if isinstance(b, float) else f"{a} {b}" for a, b in d.items()))
