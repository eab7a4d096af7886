"""frog_amd -- MI355X-native groupwise-registration hot path of valette/FROG.

Native code lives in frog_amd/csrc (HIP kernels + C ABI, C++ host); this package
is the thin Python layer tests, bench.py and the multi-process launcher use.
"""
from .pairs import Pairs            # noqa: F401
from .image_group import ImageGroup  # noqa: F401
from .volume import Staple, staple_labels  # noqa: F401
from .volume import SurfaceDistances, distance_map, surface_distances, surface_metrics  # noqa: F401
from .mesh import isosurface, read_mesh, transform_points, write_mesh  # noqa: F401
