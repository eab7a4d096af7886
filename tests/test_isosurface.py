"""The restatement of the iso-surface extractor (tests/isosurface_restate.py) against facts that do not come from the code:
closedness of all 256 cell configurations, the sphere's Euler characteristic and interpolation bound, exact ties, and label
mode as level mode on the indicator.  No device."""
import numpy as np
import pytest

import isosurface_restate as R


def test_table_shape():
    assert len(R.PERMS) == 6 and R.PERMS[0] == (0, 1, 2) and R.PERMS[5] == (2, 1, 0)
    assert R.N_TRI[0] == 0 and R.N_TRI[255] == 0
    assert R.N_TRI.max() <= 12
    # a configuration and its complement cut the same tetrahedron edges
    assert all(R.N_TRI[c] == R.N_TRI[255 - c] for c in range(256))


def test_every_cell_configuration_is_closed():
    for config in range(256):
        xyz, tri = R.isosurface(R.cell_configuration(config), level=0.5)
        if config == 0:
            assert len(xyz) == 0 and len(tri) == 0
            continue
        assert len(tri) > 0, config
        assert tri.max() < len(xyz)
        assert R.is_closed(tri), config
        assert R.signed_volume(xyz, tri) > 0, config


@pytest.mark.parametrize("case", range(len(R.SPHERES)))
def test_sphere(case):
    dims, radius, spacing, origin = R.SPHERES[case]
    f, centre = R.sphere(dims, radius, spacing, origin)
    xyz, tri = R.isosurface(f, origin, spacing, level=0.0)
    assert R.is_closed(tri)
    assert R.euler_characteristic(xyz, tri) == 2
    diagonal = float(np.sqrt(np.sum(np.square(spacing))))
    bound = diagonal ** 2 / (8 * (radius - diagonal)) + 1e-5
    error = float(np.abs(np.linalg.norm(xyz.astype(np.float64) - centre, axis=1) - radius).max())
    print("sphere %d: %d vertices, %d triangles, error %.4g, bound %.4g" % (case, len(xyz), len(tri), error, bound))
    assert error <= bound
    assert R.signed_volume(xyz, tri) > 0


def test_ties_keep_the_mesh_closed_and_the_volume_exact():
    xyz, tri = R.isosurface(R.ties_block(), level=1.0)
    assert R.is_closed(tri)
    assert R.signed_volume(xyz, tri) == 8.0
    # every vertex sits on a node of the block
    assert np.array_equal(xyz, np.round(xyz)) and xyz.min() == 1 and xyz.max() == 3


def test_label_mode_is_level_mode_on_the_indicator():
    rng = np.random.default_rng(5)
    labels = rng.integers(-2, 3, size=(6, 7, 8)).astype(np.int16)
    for value in (-2, 0, 2):
        a = R.isosurface(labels, (1, 2, 3), (0.5, 2, 1), label=value)
        b = R.isosurface((labels == value).astype(np.uint8), (1, 2, 3), (0.5, 2, 1), level=0.5)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        assert len(a[1]) > 0


def test_degenerate_grids_are_empty():
    for shape in ((1, 1, 1), (1, 5, 5), (5, 5, 1)):
        xyz, tri = R.isosurface(np.ones(shape, np.uint8), level=0.5)
        assert len(xyz) == 0 and len(tri) == 0
    xyz, tri = R.isosurface(np.zeros((3, 3, 3), np.float32), level=0.5)
    assert len(xyz) == 0 and len(tri) == 0
