"""BASELINE.json configurations at full size on the GPU.

configs[1]: 20 images x 20 000 keypoints, ~2 M pairs, linear only  -> iterations against the oracle.
configs[2]: 100 images x 20 000 keypoints, ~50 M pairs             -> one refresh, one linear and one
            deformable step against the oracle (about half a second each on the host), then
            properties that do not need the oracle: zero cross-image mean of every lattice, run-to-run
            bitwise reproducibility of a second run, sample census.
"""
import numpy as np
import pytest

from frog_amd import _abi
from frog_amd.image_group import ImageGroup
from frog_amd.pairs import Pairs
from oracle.oracle_api import OracleGroup
from gpu_util import relerr

pytestmark = pytest.mark.gpu
REL = 1e-4


def test_config2_linear_only_against_oracle():
    pairs = Pairs.synthetic(20, 20000, 10526, seed=1)          # 190 image pairs x ~10.5 k = 2.0 M pairs
    assert 1.8e6 < pairs.n_pairs < 2.2e6
    g = ImageGroup(pairs)
    ref = OracleGroup(pairs.model, _abi.FrogOptions.default())
    ref.setup_stats()
    g.setupLinearTransforms(); ref.linear_init()
    g.transformPoints(); ref.transform_points()
    assert np.array_equal(g.points()[1], ref.xyz2())
    for it in range(12):
        if it % 10 == 0:
            g.updateStats(); ref.update_stats()
            if it == 0:
                for i in range(pairs.n_images):
                    s, o = g.samples(i)
                    rs, ro = ref.samples(i)
                    assert 9000 < len(s) == len(rs) <= 10000 and np.array_equal(o, ro) and np.array_equal(s, rs)
                    assert np.array_equal(g.histogram(i), ref.histogram(i))
                    assert np.array_equal(g.em(i), ref.em(i))
        e = g.updateLinearTransforms(); er = ref.linear_step()
        g.transformPoints(); ref.transform_points()
        assert abs(e - er) / er < 1e-6
    for i in range(pairs.n_images):
        assert relerr(np.diag(g.matrix(i))[:3], np.diag(ref.matrix(i))[:3]) < 1e-6
        assert relerr(g.matrix(i)[:3, 3], ref.matrix(i)[:3, 3]) < 1e-6
    assert relerr(g.points()[1], ref.xyz2()) < 1e-6


@pytest.fixture(scope="module")
def config3():
    pairs = Pairs.synthetic(100, 20000, 10101, seed=1)         # the bench workload
    assert 4.8e7 < pairs.n_pairs < 5.2e7
    return pairs


def test_config3_steps_against_oracle(config3):
    pairs = config3
    g = ImageGroup(pairs)
    ref = OracleGroup(pairs.model, _abi.FrogOptions.default())
    ref.setup_stats()
    g.setupLinearTransforms(); ref.linear_init()
    g.transformPoints(); ref.transform_points()
    g.updateStats(); ref.update_stats()
    for i in range(0, pairs.n_images, 7):
        s, o = g.samples(i)
        rs, ro = ref.samples(i)
        assert np.array_equal(o, ro) and np.array_equal(s, rs)     # ~1 M draws per image replayed bit-exactly
        assert np.array_equal(g.em(i), ref.em(i))
    e = g.updateLinearTransforms(); er = ref.linear_step()
    assert abs(e - er) / er < 1e-6
    g.transformPoints(); ref.transform_points()
    for i in range(pairs.n_images):
        assert relerr(g.matrix(i)[:3, :], ref.matrix(i)[:3, :]) < 1e-6
    g.transformPoints(True); ref.transform_points(True)
    info = g.setupDeformableTransforms(2)
    rinfo = ref.deformable_setup(2, _abi.FrogGridInfo())
    assert list(info.dims) == list(rinfo.dims)
    g.transformPoints(); ref.transform_points()
    e = g.updateDeformableTransforms(0.02); er = ref.deformable_step(0.02)
    assert (e < 0) == (er < 0)
    if e >= 0:
        assert abs(e - er) / er < 1e-5
        for i in range(0, pairs.n_images, 9):
            assert relerr(g.grid(i, 0)[1], ref.grid(i, 0, _abi.FrogGridInfo())[1]) < REL
    assert relerr(g.point_sums(), ref.point_sums()) < 1e-5
    # the census is integer work: on identical coordinates and mixtures, 10^8 half-links, every count is equal
    g.transformPoints(); ref.transform_points()
    g.set_points2(ref.xyz2())
    for i in range(pairs.n_images):
        g.set_em(i, ref.em(i))
    cnt = g.countInliers()
    rcnt = ref.count_inliers((_abi.FrogCounts * pairs.n_images)())
    assert sum(c.pairs for c in cnt) == pairs.n_half_links
    for i in range(pairs.n_images):
        assert (cnt[i].pairs, cnt[i].inliers, cnt[i].outliers) == (rcnt[i].pairs, rcnt[i].inliers, rcnt[i].outliers)


@pytest.mark.parametrize("max_size", [10000, 20000, 700])
def test_em_prefix_sum_form_equals_term_by_term(max_size):
    """Stats::estimateDistribution on the device: the prefix-sum form of its f32 accumulators (em_scan_kernel, what
    updateStats runs) against the term-by-term form (em_kernel) on the SAME retained samples from the SAME starting
    parameters (frog_test_em_refit), over refreshes at different coordinates: cold start from (10, 300, 0.5), warm
    starts, one / two / three LDS chunks of samples (-ss 700 / 10000 / 20000).  Same bits, and the oracle agrees."""
    pairs = Pairs.synthetic(20, 20000, 10526, seed=4)
    g = ImageGroup(pairs, stats_max_size=max_size)
    ref = OracleGroup(pairs.model, _abi.FrogOptions.default(stats_max_size=max_size))
    ref.setup_stats()
    g.setupLinearTransforms(); ref.linear_init()
    g.transformPoints(); ref.transform_points()
    lib = _abi.hip_lib()
    for it in range(16):
        if it % 5 == 0:
            before = [g.em(i).copy() for i in range(pairs.n_images)]
            ref.set_xyz2(g.points()[1])
            for i in range(pairs.n_images):
                ref.set_em(i, before[i])
            g.updateStats(); ref.update_stats()
            after = [g.em(i).copy() for i in range(pairs.n_images)]
            fits = []
            for term_by_term in (1, 0):
                for i in range(pairs.n_images):
                    g.set_em(i, before[i])
                assert lib.frog_test_em_refit(g._ctx, term_by_term) == _abi.FROG_OK
                fits.append([g.em(i).copy() for i in range(pairs.n_images)])
            for i in range(pairs.n_images):
                assert np.array_equal(fits[0][i], fits[1][i]), f"image {i}, iteration {it}: {fits[0][i]} vs {fits[1][i]}"
                assert np.array_equal(after[i], fits[1][i]) and np.array_equal(after[i], ref.em(i))
        g.updateLinearTransforms(); g.transformPoints()


def _short_run(pairs):
    g = ImageGroup(pairs)
    g.linearIterations, g.deformableLevels, g.deformableIterations = 12, 2, 6
    E = g.run()
    mats = [g.matrix(i) for i in range(pairs.n_images)]
    grids = [[g.grid(i, k)[1] for k in range(g.num_grids())] for i in (0, 37, 99)]
    return g, E, mats, grids


def test_config3_properties(config3):
    pairs = config3
    g1, E1, m1, c1 = _short_run(pairs)
    # the cross-image mean is removed at every step (imageGroup.cxx:417-423): lattices sum to zero
    for k in range(g1.num_grids()):
        tot = np.zeros_like(g1.grid(0, k)[1], dtype=np.float64)
        mx = 0.0
        for i in range(pairs.n_images):
            c = g1.grid(i, k)[1]
            tot += c; mx = max(mx, float(np.max(np.abs(c))))
        assert np.max(np.abs(tot)) <= 1e-5 * max(mx, 1e-3) * pairs.n_images
    assert all(np.isfinite(E1)) and E1[11] < E1[0] and E1[-1] < E1[12]
    # reproducibility: no float atomic anywhere on the path (fixed-order sums, staged lattice flush, canonical
    # point order inside cells) -> a second run is bitwise identical, lattices included
    g2, E2, m2, c2 = _short_run(pairs)
    assert E1 == E2
    for a, b in zip(m1, m2):
        assert np.array_equal(a, b)
    for ga, gb in zip(c1, c2):
        for a, b in zip(ga, gb):
            assert np.array_equal(a, b)
    assert np.array_equal(g1.points()[1], g2.points()[1])


def test_matcher_at_pipeline_size():
    # the matching stage of the same configuration: 20 000 keypoints x 48-float descriptors per image.
    # One image pair through the oracle (4e8 candidate pairs on one host thread), several through the GPU;
    # size-independent properties for the rest: every pair passes upstream's own filters and tests.
    from frog_amd.match import Matcher, synthetic_keypoints
    from oracle.oracle_api import match_run
    imgs = synthetic_keypoints(4, 20000, seed=3)
    jobs = [(0, 1), (0, 2), (1, 3), (2, 3)]
    m = Matcher(imgs)
    got = m.run(jobs, threshold=1.0)
    (wa, wb), = match_run(imgs, jobs[:1], threshold=1.0)
    assert np.array_equal(got[0][0], wa) and np.array_equal(got[0][1], wb) and len(wa) > 10000
    for (f, s), (a, b) in zip(jobs, got):
        A, B = imgs[f], imgs[s]
        assert np.all(np.diff(b.astype(np.int64)) > 0)                          # one pair per query at most, in query order
        assert np.array_equal(A.laplacian[a], B.laplacian[b])                   # match.cpp:270
        ratio = B.scale[b] / A.scale[a]
        assert np.all(ratio.astype(np.float64) <= 1.3) and np.all((A.scale[a] / B.scale[b]).astype(np.float64) <= 1.3)   # :273-275
        d = np.sqrt(((A.desc[a].astype(np.float64) - B.desc[b]) ** 2).sum(1))
        assert np.all(d < 1.0 + 1e-5)                                           # :321
    # symmetric run: the forward half is unchanged, the reverse half lists (i, match) for the queries of `first`
    sym = m.run(jobs[:1], threshold=1.0, sym=1)[0]
    n = len(got[0][0])
    assert np.array_equal(sym[0][:n], got[0][0]) and np.array_equal(sym[1][:n], got[0][1])
    assert np.all(np.diff(sym[0][n:].astype(np.int64)) > 0)


def test_ransac_at_pipeline_size():
    # the incremental-registration stage of tools/register.py at the pipeline's keypoint count: one image of
    # 20 000 keypoints against 19 fixed ones (2.0e5 half-links), 5 000 candidates as upstream's default
    pairs = Pairs.synthetic(20, 20000, 10526, seed=1, scale_min=1.0, scale_max=1.0)
    n = pairs.n_images
    g = ImageGroup(pairs, n_fixed_images=n - 1)
    ref = OracleGroup(pairs.model, _abi.FrogOptions.default(n_fixed_images=n - 1))
    ref.setup_stats()
    g.setupLinearTransforms(); ref.linear_init()
    g.transformPoints(); ref.transform_points()
    a = g.RANSAC(n - 1, iterations=5000, batches=8)
    b = ref.ransac(n - 1, iterations=5000, batches=8)
    assert a == b > 20000                                              # an integer census: identical
    m = g.matrix(n - 1)
    assert np.allclose(m, ref.matrix(n - 1), rtol=1e-9, atol=1e-9)
    s = np.cbrt(np.linalg.det(m[:3, :3]))
    assert np.allclose(m[:3, :3] @ m[:3, :3].T, s * s * np.eye(3), atol=1e-9) and 0.9 < s < 1.1
    g.transformPoints(); ref.transform_points()
    assert np.array_equal(g.points()[1], ref.xyz2())                   # same matrix to 1e-13, f32 positions identical


def test_reslice_at_volume_size():
    # VolumeTransform's kernel on a 192^3 int16 volume through the INVERSE of a 1 + 3 link chain: identity chain = the
    # volume itself (every voxel), a slab against the oracle, and the size-independent property that resampling
    # through T^-1 and looking a voxel centre up through T meet in the same place
    from frog_amd.chain import Chain, Link, invert
    from oracle.oracle_api import chain_apply, chain_reslice
    rng = np.random.default_rng(2)
    M = np.eye(4); M[:3, 3] = [2.0, -1.0, 1.5]
    links = [Link.linear(M)]
    for k in (4, 8, 8):
        dims = (k + 3, k + 3, k + 3)
        sp = tuple(300.0 / k for _ in range(3))
        links.append(Link.bspline(dims, tuple(-s for s in sp), sp, (1.5 * rng.normal(size=(dims[0] ** 3, 3))).astype(np.float32)))
    n = 192
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    vol = (1000 + 600 * np.sin(x / 7.0) * np.cos(y / 9.0) + 3 * z).astype(np.int16)
    o, s = (0.0, 0.0, 0.0), (300.0 / n,) * 3
    assert np.array_equal(Chain([]).reslice(vol, o, s, (n, n, n), o, s, 1, -1.0), vol)
    inv = invert(links)
    c = Chain(inv)
    got = c.reslice(vol, o, s, (n, n, n), o, s, 1, -1.0)
    slab_o = (0.0, 0.0, 60 * s[2])
    want = np.clip(np.floor(chain_reslice(inv, vol, o, s, (n, n, 8), slab_o, s, 1, -1.0) + 0.5), -32768, 32767)
    assert np.abs(got[60:68] - want).max() <= 1 and (got[60:68] != want).mean() < 2e-3
    # voxel p of the output shows the source at T^-1(p): pushing that point through T must give p back
    idx = rng.integers(20, n - 20, (2000, 3))
    p = idx[:, ::-1] * np.array(s)                                      # (x, y, z) of voxel [z, y, x]
    back = chain_apply(links, c.apply(p))
    assert np.abs(back - p).max() < 2e-3                                # VTK's inverse tolerance
