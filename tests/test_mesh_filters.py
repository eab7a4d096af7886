"""The restatement of the mesh filters (tests/mesh_restate.py: Taubin smoothing and vertex clustering, include/frog_chain.h)
against facts that do not come from it: a brute-force version, meshes whose answer is known in closed form, and what the
filters do to a voxel ball.  No device."""
import numpy as np
import pytest

import isosurface_restate as IR
import mesh_restate as M

F4, F8 = np.float32, np.float64


@pytest.fixture(scope="module")
def ball():
    """(xyz, triangles, centre, xyz after 20 iterations at the defaults)."""
    xyz, tri, centre = M.blocky_ball()
    return xyz, tri, centre, M.smooth(xyz, tri)


# ---- brute force: Python sets per vertex, a loop per vertex ------------------------------------------------------------------------

def brute_neighbours(n, faces, boundary):
    times = {}
    for face in faces:
        face = [int(i) for i in face]
        for k in range(len(face)):
            a, b = face[k], face[(k + 1) % len(face)]
            if a != b:
                times[frozenset((a, b))] = times.get(frozenset((a, b)), 0) + 1
    around, border = [set() for _ in range(n)], [set() for _ in range(n)]
    for pair, count in times.items():
        a, b = tuple(pair)
        around[a].add(b); around[b].add(a)
        if count == 1:
            border[a].add(b); border[b].add(a)
    return [sorted(around[v]) if not border[v] else (sorted(border[v]) if boundary else []) for v in range(n)]


def brute_smooth(xyz, faces, iterations, lam, mu, boundary):
    x = np.array(xyz, F4)
    if iterations == 0 or (lam == 0 and mu == 0):
        return x
    around = brute_neighbours(len(x), faces, boundary)
    for it in range(2 * iterations):
        f, new = F8(mu if it % 2 else lam), x.copy()
        for v, ring in enumerate(around):
            if not ring:
                continue
            for axis in range(3):
                s = F8(0.0)
                for w in ring:
                    s = s + F8(x[w, axis])
                m = s / F8(len(ring))
                new[v, axis] = F4(F8(x[v, axis]) + f * (m - F8(x[v, axis])))
        x = new
    return x


def brute_cluster(xyz, tri, cell):
    x = np.asarray(xyz, F4)
    lo = [min(float(p[a]) for p in x) for a in range(3)]
    cells = [tuple(int(np.floor((float(p[a]) - lo[a]) / cell)) for a in range(3)) for p in x]
    order = sorted(set(cells), key=lambda c: (c[2], c[1], c[0]))
    index = {c: k for k, c in enumerate(order)}
    cluster_of = np.array([index[c] for c in cells], np.uint32)
    new = np.zeros((len(order), 3), F4)
    for k in range(len(order)):
        for a in range(3):
            s, count = F8(0.0), 0
            for v in range(len(x)):
                if cluster_of[v] == k:
                    s, count = s + F8(x[v, a]), count + 1
            new[k, a] = F4(s / F8(count))
    out = [[cluster_of[i] for i in t] for t in tri if len({int(cluster_of[i]) for i in t}) == 3]
    return new, np.array(out, np.uint32).reshape(-1, 3), cluster_of


def test_restatement_equals_brute_force_on_the_ball(ball):
    xyz, tri, _, _ = ball
    for how in (dict(iterations=2, lam=0.5, mu=-0.53, boundary=1), dict(iterations=1, lam=0.5, mu=0.5, boundary=0)):
        assert M.smooth(xyz, tri, **how).tobytes() == brute_smooth(xyz, tri, **how).tobytes()
    # an open piece of it, so that both boundary rules act
    piece = tri[:900]
    for boundary in (0, 1):
        got = M.smooth(xyz, piece, 2, 0.5, -0.53, boundary)
        assert got.tobytes() == brute_smooth(xyz, piece, 2, 0.5, -0.53, boundary).tobytes()
        assert got.tobytes() != xyz.tobytes()
    got, want = M.cluster(xyz[:600], tri[(tri < 600).all(axis=1)], 2.0), brute_cluster(xyz[:600], tri[(tri < 600).all(axis=1)], 2.0)
    assert all(g.tobytes() == w.tobytes() and g.shape == w.shape for g, w in zip(got, want))


def test_restatement_on_polygons_and_odd_faces():
    rng = np.random.default_rng(2)
    xyz = rng.standard_normal((9, 3)).astype(F4)
    faces = [[0, 1, 2, 3], [3, 2, 4, 5, 6], [1, 7, 2], [1, 2, 7], [2, 2, 8], [5], [6, 0]]
    for boundary in (0, 1):
        assert M.smooth(xyz, faces, 3, 0.5, -0.53, boundary).tobytes() == brute_smooth(xyz, faces, 3, 0.5, -0.53, boundary).tobytes()


# ---- closed forms -------------------------------------------------------------------------------------------------------------------

def test_octahedron_shrinks_by_three_quarters():
    xyz, tri = M.octahedron(8.0)
    assert IR.is_closed(tri) and IR.euler_characteristic(xyz, tri) == 2
    # lambda: x - 0.5 x = 0.5 x; mu = -0.5: 0.5 x + 0.5 * 0.5 x = 0.75 x, every step exact
    assert M.smooth(xyz, tri, 1, 0.5, -0.5).tobytes() == (xyz * F4(0.75)).tobytes()


def test_flat_grid():
    """An interior vertex's six neighbours sum to six times itself, exactly, and a border vertex between two others is their
    mean: with a pinned border nothing ever moves.  With a sliding border only the four corners move in a pass, so every
    interior vertex keeps its bytes in every pass whose neighbours have not moved yet: all 16 in the first pass, and after a
    whole iteration (two passes) all but the two that the cut diagonal joins to a corner, (1, 1) and (4, 4)."""
    xyz, tri = M.grid(6, 6)
    assert M.smooth(xyz, tri, 5, 0.5, -0.53, boundary=0).tobytes() == xyz.tobytes()
    interior = ((xyz[:, 0] > 0) & (xyz[:, 0] < 5) & (xyz[:, 1] > 0) & (xyz[:, 1] < 5))
    corners = np.isin(xyz[:, 0], (0, 5)) & np.isin(xyz[:, 1], (0, 5))
    assert interior.sum() == 16 and corners.sum() == 4
    first = M.one_pass(xyz, *M.neighbours(len(xyz), tri, 1), 0.5)
    assert first[~corners].tobytes() == xyz[~corners].tobytes() and (first[corners] != xyz[corners]).any(axis=1).all()
    moved = M.smooth(xyz, tri, 1, 0.5, -0.53, boundary=1)
    beside_a_corner = np.isin(np.arange(36), (7, 28))
    assert moved[interior & ~beside_a_corner].tobytes() == xyz[interior & ~beside_a_corner].tobytes()
    assert (moved[beside_a_corner] != xyz[beside_a_corner]).any(axis=1).all()


def test_identity_and_faces_untouched(ball):
    xyz, tri, _, _ = ball
    with_zero = xyz.copy()
    with_zero[0, 0] = -0.0                  # a pass would turn it into +0
    before = tri.copy()
    assert M.smooth(with_zero, tri, 0, 0.5, -0.53).tobytes() == with_zero.tobytes()
    assert M.smooth(with_zero, tri, 7, 0.0, -0.0).tobytes() == with_zero.tobytes()
    assert tri.tobytes() == before.tobytes()


# ---- the blocky ball ------------------------------------------------------------------------------------------------------------------

def test_ball_taubin_smooths_without_shrinking(ball):
    xyz, tri, centre, smooth = ball
    assert (len(xyz), len(tri)) == (3830, 7656) and IR.is_closed(tri) and IR.euler_characteristic(xyz, tri) == 2
    assert (np.modf(xyz * 2)[0] == 0).all()            # label mode: every vertex on an edge midpoint
    raw_sd, smooth_sd = M.radial_stdev(xyz, centre), M.radial_stdev(smooth, centre)
    raw_volume, smooth_volume = IR.signed_volume(xyz, tri), IR.signed_volume(smooth, tri)
    laplace_volume = IR.signed_volume(M.smooth(xyz, tri, 20, 0.5, 0.5), tri)
    print("radial stdev %.4f -> %.4f (ratio %.3f); volume %.1f -> Taubin %.1f (%+.2f %%), Laplacian %.1f (%+.1f %%)"
          % (raw_sd, smooth_sd, smooth_sd / raw_sd, raw_volume, smooth_volume, 100 * (smooth_volume / raw_volume - 1),
             laplace_volume, 100 * (laplace_volume / raw_volume - 1)))
    assert smooth_sd / raw_sd <= 0.70
    assert abs(smooth_volume / raw_volume - 1) <= 0.01
    assert laplace_volume < 0.90 * raw_volume
    assert IR.is_closed(tri) and IR.euler_characteristic(smooth, tri) == 2


def test_ball_clustered(ball):
    _, tri, _, smooth = ball
    cell = 2.0
    xyz, out, cluster_of = M.cluster(smooth, tri, cell)
    lo = smooth.min(axis=0).astype(F8)
    cells = np.unique(np.floor((smooth.astype(F8) - lo) / cell), axis=0)
    assert len(xyz) == len(cells) and cluster_of.max() == len(xyz) - 1
    assert M.edges_balanced(out)
    move = np.linalg.norm(smooth.astype(F8) - xyz[cluster_of].astype(F8), axis=1).max()
    print("cell %.1f: %d vertices, %d triangles from %d and %d; largest move %.3f (bound %.3f); closed 2-manifold: %s"
          % (cell, len(xyz), len(out), len(smooth), len(tri), move, cell * np.sqrt(3), IR.is_closed(out)))
    assert move <= cell * np.sqrt(3) + 1e-5
    assert 0 < len(out) < len(tri) and out.max() < len(xyz)


def test_cluster_cell_sizes(ball):
    _, tri, _, smooth = ball
    d = smooth.astype(F8)
    smallest = np.inf                                   # the smallest separation of any two vertices, all pairs
    for start in range(0, len(d), 256):
        gap = np.linalg.norm(d[start:start + 256, None, :] - d[None, :, :], axis=2)
        gap[np.arange(len(gap)), start + np.arange(len(gap))] = np.inf
        smallest = min(smallest, gap.min())
    assert smallest > 1e-3
    xyz, out, cluster_of = M.cluster(smooth, tri, smallest / 2)     # a cell's diagonal is below the separation: nothing merges
    assert len(out) == len(tri) and sorted(map(tuple, xyz.tolist())) == sorted(map(tuple, smooth.tolist()))
    assert np.array_equal(xyz[cluster_of], smooth)
    xyz, out, cluster_of = M.cluster(smooth, tri, 1000.0)
    assert xyz.shape == (1, 3) and out.shape == (0, 3) and not cluster_of.any()
    assert np.allclose(xyz[0], d.mean(axis=0), atol=1e-5)


def test_cluster_keys_pass_32_bits():
    xyz, tri = M.far_apart()
    step, top = 2.0 ** 20, 2.0 ** 21 - 1
    new, out, cluster_of = M.cluster(xyz, tri, 1.0)
    # 2^21 cells per axis, the most that is accepted; the second vertex's key is (2^20 * 2^21 + 2^20) * 2^21 + 2^20 > 2^61
    assert cluster_of.tolist() == [0, 1, 2, 1] and out.tolist() == [[0, 1, 2], [2, 1, 0]]
    assert new[1].tolist() == [step, step, step + 0.125] and new[2].tolist() == [top] * 3


def test_cluster_refusals():
    xyz, tri = M.octahedron(8.0)
    for cell in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            M.cluster(xyz, tri, cell)
    with pytest.raises(ValueError):
        M.cluster(xyz, tri, 16.0 / 2 ** 21 * 0.99)      # 2^21 / 0.99 cells on an axis
    M.cluster(xyz, tri, 16.0 / (2 ** 21 - 1))           # exactly 2^21: accepted
    bad = xyz.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError):
        M.cluster(bad, tri, 1.0)
    with pytest.raises(ValueError):
        M.cluster(xyz, np.array([[0, 1, 2, 3]], np.uint32), 1.0)
    with pytest.raises(ValueError):
        M.cluster(xyz, np.array([[0, 1, 6]], np.uint32), 1.0)
    with pytest.raises(ValueError):
        M.smooth(xyz, np.array([[0, 1, 6]], np.uint32))
    assert all(len(a) == 0 for a in M.cluster(np.zeros((0, 3), F4), np.zeros((0, 3), np.uint32), 1.0))
