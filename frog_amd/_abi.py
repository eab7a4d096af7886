"""ctypes view of include/frog_types.h, include/frog_hip.h and include/frog_host.h.

The shared libraries are built in-tree by ``__graft_entry__.build()`` (or
``make -C frog_amd/csrc``).  Loading fails loudly when they are missing: there is
no Python or CPU stand-in for the HIP path.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, "lib")



def usable_cpus():
    """CPUs this process may run on: the affinity mask capped by the cgroup quota (csrc/common/usable_cpus.h, the same rule).
    On the GPU boxes os.cpu_count() says 256 and cpu.max says 16: 256 OpenMP threads there are throttled together."""
    import math
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)

    def quota(d):
        try:
            with open(os.path.join(d, "cpu.max")) as fh:
                q, p = fh.read().split()[:2]
            return None if q == "max" else float(q) / float(p)
        except (OSError, ValueError):
            pass
        try:
            with open(os.path.join(d, "cpu.cfs_quota_us")) as fh:
                q = float(fh.read())
            with open(os.path.join(d, "cpu.cfs_period_us")) as fh:
                p = float(fh.read())
            return q / p if q > 0 and p > 0 else None
        except (OSError, ValueError):
            return None
    dirs = ["/sys/fs/cgroup", "/sys/fs/cgroup/cpu"]
    try:
        with open("/proc/self/cgroup") as fh:
            for line in fh:
                _, ctrl, path = line.rstrip("\n").split(":", 2)
                root = "/sys/fs/cgroup" if ctrl == "" else ("/sys/fs/cgroup/cpu" if "cpu" in ctrl.split(",") or "cpuacct" in ctrl.split(",") else None)
                while root and len(path) > 1:
                    dirs.append(root + path)
                    path = path.rsplit("/", 1)[0] or "/"
    except (OSError, ValueError):
        pass
    for d in dirs:
        q = quota(d)
        if q and q > 0:
            n = min(n, max(1, math.ceil(q - 1e-9)))
    return max(1, n)


def device_source_hash():
    """sha256 (first 16 hex digits) over the HIP sources of the registration kernels (everything under csrc/device
    except the matcher, the transform chains with their rank kernels and the collectives library), in name order: what a PMC measurement under
    profiles/ is keyed on, so that bench.py can tell when the kernels have changed since."""
    import hashlib
    d = os.path.join(_HERE, "csrc", "device")
    h = hashlib.sha256()
    for name in sorted(os.listdir(d)):
        if name.endswith((".hip", ".h")) and name not in ("comm.hip", "match.hip", "chain.hip", "k_rank.hip.h"):
            h.update(name.encode())
            with open(os.path.join(d, name), "rb") as fh:
                h.update(fh.read())
    return h.hexdigest()[:16]


c_float_p = C.POINTER(C.c_float)
c_double_p = C.POINTER(C.c_double)
c_u32_p = C.POINTER(C.c_uint32)


class FrogModel(C.Structure):
    """frog_model (include/frog_types.h)."""
    _fields_ = [("n_images", C.c_uint32),
                ("point_offset", C.c_void_p),
                ("xyz", C.c_void_p),
                ("row_ptr", C.c_void_p),
                ("link_image", C.c_void_p),
                ("link_point", C.c_void_p)]


class FrogOptions(C.Structure):
    """frog_options; defaults = imageGroup.h:52-82, stats.cxx:10-12."""
    _fields_ = [("linear_alpha", C.c_float),
                ("use_scale", C.c_int32),
                ("initial_grid_size", C.c_float),
                ("bounding_box_margin", C.c_float),
                ("inlier_threshold", C.c_float),
                ("guarantee_diffeomorphism", C.c_int32),
                ("max_displacement_ratio", C.c_float),
                ("stats_max_size", C.c_int32),
                ("stats_max_iterations", C.c_int32),
                ("stats_epsilon", C.c_float),
                ("n_fixed_images", C.c_int32),
                ("max_levels_hint", C.c_int32),
                ("reference_order", C.c_int32),
                ("selections_in_background", C.c_int32),
                ("reserved", C.c_int32 * 2)]

    @classmethod
    def default(cls, **kw):
        o = cls(0.5, 1, 100.0, 0.1, 0.5, 1, 0.4, 10000, 10000, 1e-6)
        for k, v in kw.items():
            if not hasattr(o, k):
                raise AttributeError(k)
            setattr(o, k, v)
        return o


class FrogGridInfo(C.Structure):
    _fields_ = [("dims", C.c_int32 * 3),
                ("n_grid", C.c_int32),
                ("origin", C.c_double * 3),
                ("spacing", C.c_double * 3),
                ("bbox", C.c_double * 6)]


class FrogRansacOptions(C.Structure):
    """frog_ransac_options; defaults = imageGroup.h:70-74."""
    _fields_ = [("iterations", C.c_int32), ("batches", C.c_int32),
                ("inlier_distance", C.c_float), ("max_scale", C.c_float)]


class FrogCounts(C.Structure):
    _fields_ = [("points", C.c_int64), ("pairs", C.c_int64),
                ("inliers", C.c_int64), ("outliers", C.c_int64),
                ("c1", C.c_float), ("c2", C.c_float), ("ratio", C.c_float), ("pad_", C.c_float)]


class FrogSynthParams(C.Structure):
    _fields_ = [("n_images", C.c_uint32),
                ("points_per_image", C.c_uint32),
                ("n_landmarks", C.c_uint32),
                ("pairs_per_block", C.c_double),
                ("partners_per_image", C.c_uint32),
                ("outlier_fraction", C.c_float),
                ("noise_sigma", C.c_float),
                ("bump_amplitude", C.c_float),
                ("scale_min", C.c_float),
                ("scale_max", C.c_float),
                ("translation_range", C.c_float),
                ("seed", C.c_uint64)]


class FrogKernelTime(C.Structure):
    _fields_ = [("ms_total", C.c_double), ("launches", C.c_uint64)]


SCHEDULE_MAX_LEVELS, SCHEDULE_MAX_LATTICES, FROG_K_COUNT = 16, 512, 10


class FrogSchedulePlan(C.Structure):
    """frog_schedule_plan (include/frog_host.h)."""
    _fields_ = [("plan_bytes", C.c_uint32), ("result_bytes", C.c_uint32),
                ("warmup_linear", C.c_int32), ("linear", C.c_int32), ("n_levels", C.c_int32),
                ("per_level", C.c_int32 * SCHEDULE_MAX_LEVELS), ("stat_interval", C.c_int32),
                ("deformable_alpha", C.c_float), ("anchor", C.c_float * 3), ("profile", C.c_int32), ("time_comm", C.c_int32),
                ("proxy_xyz2", C.c_void_p), ("proxy_em", C.c_void_p)]


class FrogScheduleLattice(C.Structure):
    _fields_ = [("level", C.c_int32), ("dims", C.c_int32 * 3), ("iterations", C.c_int32), ("setup_host_s", C.c_double)]


class FrogScheduleResult(C.Structure):
    """frog_schedule_result (include/frog_host.h)."""
    _fields_ = [("elapsed_s", C.c_double), ("phase_s", C.c_double * (1 + SCHEDULE_MAX_LEVELS)),
                ("iterations", C.c_int32), ("grids_per_level", C.c_int32 * SCHEDULE_MAX_LEVELS), ("n_lattices", C.c_int32),
                ("lattices", FrogScheduleLattice * SCHEDULE_MAX_LATTICES), ("final_E", C.c_double),
                ("kernels", FrogKernelTime * FROG_K_COUNT),
                ("kernels_by_phase", (FrogKernelTime * FROG_K_COUNT) * (1 + SCHEDULE_MAX_LEVELS)),
                ("comm_ms", C.c_double * 4), ("comm_calls", C.c_uint64 * 4), ("comm_sampled", C.c_uint64 * 4),
                ("replica_hash", C.c_uint64)]


FROG_K_NAMES = ["sweep_linear", "sweep_deformable", "scatter", "lattice", "transform", "stats", "combine", "cull", "sweep_build", "sweep_linear_build"]
FROG_OK, FROG_E_INVALID, FROG_E_NODEVICE, FROG_E_HIP, FROG_E_STATE, FROG_E_NOMEM, FROG_E_IO = range(7)
FROG_BUF_XYZ2, FROG_BUF_EM, FROG_BUF_ENERGY, FROG_BUF_GRIDSUM = range(4)

# name -> (restype, argtypes): every symbol include/frog_hip.h declares
class FrogKeypoints(C.Structure):
    """frog_keypoints (include/frog_match.h): host arrays of one image's keypoints."""
    _fields_ = [("n", C.c_uint32), ("dim", C.c_uint32), ("xyz", c_float_p), ("scale", c_float_p),
                ("laplacian", c_float_p), ("response", c_float_p), ("desc", c_float_p)]


class FrogVolume(C.Structure):
    """frog_volume (include/frog_chain.h)."""
    _fields_ = [("dims", C.c_uint32 * 3), ("spacing", C.c_double * 3), ("origin", C.c_double * 3),
                ("dtype", C.c_int), ("data", C.c_void_p)]


class FrogMesh(C.Structure):
    """frog_mesh (include/frog_host.h)."""
    _fields_ = [("n_points", C.c_uint32), ("xyz", c_float_p), ("n_faces", C.c_uint32), ("face_ptr", C.POINTER(C.c_uint32)),
                ("face_idx", C.POINTER(C.c_uint32))]


FROG_ISO_LEVEL, FROG_ISO_LABEL = 0, 1   # include/frog_chain.h

FROG_V_DTYPES = ["uint8", "int8", "uint16", "int16", "uint32", "int32", "float32", "float64"]


def volume_view(a, origin, spacing, dims=None):
    """FrogVolume over the C-contiguous array a[z, y, x], which must outlive it; with a = None, the bare grid of
    dims(x, y, z): float32, no voxels."""
    if a is not None and (a.ndim != 3 or a.dtype.name not in FROG_V_DTYPES):
        raise ValueError("3-D scalar volume of a supported type expected")
    v = FrogVolume()
    v.dims[:] = [int(d) for d in (dims if a is None else a.shape[::-1])]; v.origin[:] = origin; v.spacing[:] = spacing
    v.dtype = FROG_V_DTYPES.index("float32" if a is None else a.dtype.name)
    v.data = None if a is None else a.ctypes.data
    return v


def grid_triplet(origin, spacing, dims):
    """(origin, spacing, dims) of a grid as the C arrays frog_chain_check and frog_chain_sample take."""
    return (C.c_double * 3)(*origin), (C.c_double * 3)(*spacing), (C.c_uint32 * 3)(*dims)


FROG_RANK_MAX_IMAGES = 4096         # include/frog_chain.h: the capacity of frog_rank's sort kernels
FROG_GLM_MAX_IMAGES, FROG_GLM_MAX_COLUMNS, FROG_GLM_MAX_CONTRASTS = 4096, 8, 8     # include/frog_chain.h: frog_glm's limits
FROG_SMOOTH_MAX_RADIUS, FROG_SMOOTH_FWHM = 64, 2.3548200450309493                  # include/frog_chain.h: fwhm = FROG_SMOOTH_FWHM * sigma
FROG_MODES_MAX_IMAGES, FROG_MODES_CHUNK = 512, 1024                                # include/frog_chain.h: frog_modes' limit and chunk


class FrogScoreSums(C.Structure):
    """frog_score_sums (include/frog_chain.h)."""
    _fields_ = [("n", C.c_uint64), ("n_nonfinite", C.c_uint64), ("sx", C.c_double), ("sy", C.c_double), ("sxx", C.c_double),
                ("syy", C.c_double), ("sxy", C.c_double), ("sad", C.c_double)]


FROG_SURFACE_MAX_LABELS = 256      # include/frog_chain.h: the most values a frog_surface measures


class FrogSurfaceRow(C.Structure):
    """frog_surface_row (include/frog_chain.h)."""
    _fields_ = [("n_a", C.c_uint64), ("n_b", C.c_uint64), ("sum_ab", C.c_uint64), ("sum_ba", C.c_uint64),
                ("max_ab", C.c_uint32), ("max_ba", C.c_uint32), ("pct_ab", C.c_uint32), ("pct_ba", C.c_uint32)]


class FrogScoreMetrics(C.Structure):
    """frog_score_metrics (include/frog_host.h)."""
    _fields_ = [("ncc", C.c_double), ("mean_abs_diff", C.c_double), ("rmse", C.c_double), ("mi", C.c_double), ("nmi", C.c_double)]


class FrogChainLink(C.Structure):
    """frog_chain_link (include/frog_chain.h)."""
    _fields_ = [("type", C.c_int), ("matrix", C.c_double * 16), ("dims", C.c_uint32 * 3), ("origin", C.c_double * 3),
                ("spacing", C.c_double * 3), ("coeffs", c_float_p)]


class FrogMatchOptions(C.Structure):
    _fields_ = [("threshold", C.c_float), ("dist2second", C.c_float), ("anat", C.c_float), ("sym", C.c_int),
                ("all", C.c_int), ("reserved", C.c_int * 3)]

    @classmethod
    def default(cls, **kw):
        o = cls()
        hip_lib().frog_match_options_default(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o


HIP_SYMBOLS = {
    "frog_device_warm": (C.c_int, [C.c_int]),
    "frog_device_count": (C.c_int, []),
    "frog_last_error": (C.c_char_p, []),
    "frog_create": (C.c_int, [C.POINTER(FrogModel), C.POINTER(FrogOptions), C.c_int, C.c_uint32, C.c_uint32,
                              C.POINTER(C.c_void_p)]),
    "frog_destroy": (None, [C.c_void_p]),
    "frog_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "frog_synchronize": (C.c_int, [C.c_void_p]),
    "frog_linear_init": (C.c_int, [C.c_void_p, c_float_p]),
    "frog_transform_points": (C.c_int, [C.c_void_p, C.c_int]),
    "frog_update_stats": (C.c_int, [C.c_void_p]),
    "frog_linear_step": (C.c_int, [C.c_void_p, c_double_p]),
    "frog_ransac": (C.c_int, [C.c_void_p, C.POINTER(FrogModel), C.c_uint32, C.POINTER(FrogRansacOptions),
                              C.POINTER(C.c_int64)]),
    "frog_deformable_setup": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(FrogGridInfo)]),
    "frog_deformable_step": (C.c_int, [C.c_void_p, C.c_float, c_double_p]),
    "frog_count_inliers": (C.c_int, [C.c_void_p, C.POINTER(FrogCounts)]),
    "frog_num_points": (C.c_uint64, [C.c_void_p]),
    "frog_num_images": (C.c_uint32, [C.c_void_p]),
    "frog_get_points": (C.c_int, [C.c_void_p, c_float_p, c_float_p]),
    "frog_set_points2": (C.c_int, [C.c_void_p, c_float_p]),
    "frog_get_linear": (C.c_int, [C.c_void_p, C.c_uint32, c_double_p]),
    "frog_get_em": (C.c_int, [C.c_void_p, C.c_uint32, c_float_p]),
    "frog_set_em": (C.c_int, [C.c_void_p, C.c_uint32, c_float_p]),
    "frog_set_em_rows": (C.c_int, [C.c_void_p, c_float_p, C.c_uint32, C.c_uint32]),
    "frog_get_samples": (C.c_int, [C.c_void_p, C.c_uint32, c_float_p, c_u32_p, C.c_int, C.POINTER(C.c_int)]),
    "frog_get_histogram": (C.c_int, [C.c_void_p, C.c_uint32, c_float_p, C.c_int, C.POINTER(C.c_int)]),
    "frog_num_grids": (C.c_int, [C.c_void_p]),
    "frog_get_grid": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(FrogGridInfo), c_float_p, C.c_size_t]),
    "frog_get_point_sums": (C.c_int, [C.c_void_p, c_float_p]),
    "frog_get_gradient": (C.c_int, [C.c_void_p, C.c_uint32, c_float_p, C.c_size_t]),
    "frog_chain_create": (C.c_int, [C.POINTER(FrogChainLink), C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]),
    "frog_chain_destroy": (None, [C.c_void_p]),
    "frog_chain_num_links": (C.c_uint32, [C.c_void_p]),
    "frog_chain_apply": (C.c_int, [C.c_void_p, c_double_p, c_double_p, C.c_size_t]),
    "frog_chain_check": (C.c_int, [C.c_void_p, c_double_p, c_double_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                   c_double_p]),
    "frog_chain_sample": (C.c_int, [C.c_void_p, c_double_p, c_double_p, C.POINTER(C.c_uint32), C.c_int, C.c_void_p, C.c_void_p]),
    "frog_chain_invert_links": (C.c_int, [C.POINTER(FrogChainLink), C.c_uint32, C.POINTER(FrogChainLink)]),
    "frog_chain_reslice": (C.c_int, [C.c_void_p, C.POINTER(FrogVolume), C.POINTER(FrogVolume), C.c_int, C.c_double]),
    "frog_average_create": (C.c_int, [C.POINTER(FrogVolume), C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]),
    "frog_average_add": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(FrogVolume), C.c_int, C.c_double, C.POINTER(FrogVolume)]),
    "frog_average_finish": (C.c_int, [C.c_void_p, c_float_p, c_float_p]),
    "frog_average_destroy": (None, [C.c_void_p]),
    "frog_cover_create": (C.c_int, [C.POINTER(FrogVolume), C.c_int, C.POINTER(C.c_void_p)]),
    "frog_cover_add": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(FrogVolume), C.POINTER(FrogVolume), C.c_int, C.c_double,
                                 C.POINTER(FrogVolume)]),
    "frog_cover_finish": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, c_float_p, c_float_p, C.POINTER(C.c_uint16)]),
    "frog_cover_score": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(FrogVolume), C.POINTER(FrogVolume), C.c_int, C.c_double,
                                   C.c_uint32, C.c_int, C.c_uint32, C.c_float, C.c_float, C.POINTER(FrogScoreSums),
                                   C.POINTER(C.c_uint64)]),
    "frog_cover_destroy": (None, [C.c_void_p]),
    "frog_rank_planes": (C.c_int, [C.POINTER(FrogVolume), C.c_uint32, C.c_int, C.POINTER(C.c_uint32)]),
    "frog_rank_create": (C.c_int, [C.POINTER(FrogVolume), C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]),
    "frog_rank_add": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(FrogVolume), C.POINTER(FrogVolume), C.c_int, C.c_double]),
    "frog_rank_finish": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.POINTER(C.c_double), c_float_p, c_float_p,
                                   C.POINTER(C.c_uint16)]),
    "frog_rank_destroy": (None, [C.c_void_p]),
    "frog_glm_planes": (C.c_int, [C.POINTER(FrogVolume), C.c_uint32, C.c_int, C.POINTER(C.c_uint32)]),
    "frog_glm_create": (C.c_int, [C.POINTER(FrogVolume), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, c_double_p, C.c_int,
                                  C.POINTER(C.c_void_p)]),
    "frog_glm_add": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(FrogVolume), C.POINTER(FrogVolume), C.c_int, C.c_double]),
    "frog_glm_add_jacobian": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(FrogVolume), C.POINTER(FrogVolume), C.c_int]),
    "frog_glm_plane": (C.c_int, [C.c_void_p, C.c_uint32, c_float_p]),
    "frog_glm_finish": (C.c_int, [C.c_void_p, C.c_uint32, c_double_p, C.c_uint32, C.c_double, C.POINTER(C.c_uint8), C.c_float,
                                  c_float_p, c_float_p, c_float_p, C.POINTER(C.c_uint16)]),
    "frog_glm_permute": (C.c_int, [C.c_void_p, C.c_uint32, c_double_p, C.c_uint32, C.c_double, C.POINTER(C.c_uint8), C.c_uint32,
                                   C.c_uint32, c_u32_p, C.POINTER(C.c_int8), c_float_p, c_float_p]),
    "frog_glm_draw": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, C.c_int, c_u32_p, C.POINTER(C.c_int8)]),
    "frog_glm_destroy": (None, [C.c_void_p]),
    "frog_components": (C.c_int, [C.POINTER(FrogVolume), C.c_int, C.c_int, c_u32_p, c_u32_p, C.POINTER(C.c_uint64)]),
    "frog_clusters_create": (C.c_int, [C.POINTER(FrogVolume), C.c_uint32, C.c_uint32, C.c_int, C.c_float, C.c_int, C.c_int,
                                       C.POINTER(C.c_void_p)]),
    "frog_glm_permute_clusters": (C.c_int, [C.c_void_p, C.c_uint32, c_double_p, C.c_uint32, C.c_double, C.POINTER(C.c_uint8), C.c_uint32,
                                            C.c_uint32, c_u32_p, C.POINTER(C.c_int8), C.c_uint32, C.c_void_p, c_float_p, c_float_p]),
    "frog_clusters_finish": (C.c_int, [C.c_void_p, c_u32_p]),
    "frog_clusters_mask": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_uint8)]),
    "frog_clusters_labels": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, c_u32_p, c_u32_p]),
    "frog_clusters_destroy": (None, [C.c_void_p]),
    "frog_tfce_volume": (C.c_int, [C.POINTER(FrogVolume), C.c_int, C.c_float, C.c_double, C.c_double, C.c_int, C.c_int, c_float_p, c_float_p]),
    "frog_tfce_create": (C.c_int, [C.POINTER(FrogVolume), C.c_uint32, C.c_uint32, C.c_int, C.c_float, C.c_double, C.c_double, C.c_int, C.c_int,
                                   C.POINTER(C.c_void_p)]),
    "frog_glm_permute_tfce": (C.c_int, [C.c_void_p, C.c_uint32, c_double_p, C.c_uint32, C.c_double, C.POINTER(C.c_uint8), C.c_uint32,
                                        C.c_uint32, c_u32_p, C.POINTER(C.c_int8), C.c_uint32, C.c_void_p, c_float_p, c_float_p]),
    "frog_tfce_finish": (C.c_int, [C.c_void_p, c_float_p]),
    "frog_tfce_levels": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_uint8)]),
    "frog_tfce_map": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, c_float_p]),
    "frog_tfce_destroy": (None, [C.c_void_p]),
    "frog_smooth_taps": (C.c_int, [C.c_double, C.c_double, c_u32_p, c_double_p]),
    "frog_smooth_volume": (C.c_int, [C.POINTER(FrogVolume), C.POINTER(C.c_uint8), C.c_double, C.c_int, c_float_p]),
    "frog_glm_smooth": (C.c_int, [C.c_void_p, C.c_double]),
    "frog_glm_smooth_planes": (C.c_int, [C.POINTER(FrogVolume), C.c_uint32, C.c_double, C.c_int, C.POINTER(C.c_uint32)]),
    "frog_modes_planes": (C.c_int, [C.POINTER(FrogVolume), C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_uint32)]),
    "frog_modes_create": (C.c_int, [C.POINTER(FrogVolume), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]),
    "frog_modes_add_displacement": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(FrogVolume), C.POINTER(FrogVolume)]),
    "frog_modes_add_jacobian": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(FrogVolume), C.POINTER(FrogVolume), C.c_int]),
    "frog_modes_add": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(FrogVolume), C.POINTER(FrogVolume), C.c_int, C.c_double]),
    "frog_modes_plane": (C.c_int, [C.c_void_p, C.c_uint32, c_float_p]),
    "frog_modes_gram": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), c_double_p, C.POINTER(C.c_uint64)]),
    "frog_modes_project": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.c_uint32, c_double_p, C.c_float, c_float_p, c_float_p]),
    "frog_modes_eigen": (C.c_int, [C.c_uint32, c_double_p, C.c_double, c_double_p, c_double_p]),
    "frog_modes_destroy": (None, [C.c_void_p]),
    "frog_labels_create": (C.c_int, [C.POINTER(FrogVolume), C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]),
    "frog_labels_add": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(FrogVolume), C.c_double, C.POINTER(FrogVolume)]),
    "frog_labels_finish": (C.c_int, [C.c_void_p, c_u32_p]),
    "frog_labels_table": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "frog_labels_fused": (C.c_int, [C.c_void_p, C.POINTER(FrogVolume), c_float_p]),
    "frog_labels_probability": (C.c_int, [C.c_void_p, C.c_int64, c_float_p]),
    "frog_labels_destroy": (None, [C.c_void_p]),
    "frog_staple_create": (C.c_int, [C.POINTER(FrogVolume), C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]),
    "frog_staple_add": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(FrogVolume), C.c_double, C.POINTER(FrogVolume)]),
    "frog_staple_finish": (C.c_int, [C.c_void_p, c_u32_p]),
    "frog_staple_values": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "frog_staple_solve": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_uint32, C.c_int, c_u32_p, c_double_p,
                                    C.POINTER(C.c_uint64)]),
    "frog_staple_fused": (C.c_int, [C.c_void_p, C.POINTER(FrogVolume), c_float_p]),
    "frog_staple_probability": (C.c_int, [C.c_void_p, C.c_int64, c_float_p]),
    "frog_staple_performance": (C.c_int, [C.c_void_p, c_double_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), c_double_p]),
    "frog_staple_destroy": (None, [C.c_void_p]),
    "frog_wlabels_create": (C.c_int, [C.POINTER(FrogVolume), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_int,
                                      C.POINTER(C.c_void_p)]),
    "frog_wlabels_target": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(FrogVolume), C.c_int, C.c_double, C.POINTER(FrogVolume)]),
    "frog_wlabels_add": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(FrogVolume), C.POINTER(FrogVolume), C.c_int, C.c_double,
                                   C.c_double, C.POINTER(FrogVolume), C.POINTER(FrogVolume)]),
    "frog_wlabels_finish": (C.c_int, [C.c_void_p, c_u32_p]),
    "frog_wlabels_values": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "frog_wlabels_fused": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(FrogVolume), c_float_p]),
    "frog_wlabels_probability": (C.c_int, [C.c_void_p, C.c_int64, c_float_p]),
    "frog_wlabels_destroy": (None, [C.c_void_p]),
    "frog_jlabels_create": (C.c_int, [C.POINTER(FrogVolume), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_int, C.c_int,
                                      C.POINTER(C.c_void_p)]),
    "frog_jlabels_target": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(FrogVolume), C.c_int, C.c_double, C.POINTER(FrogVolume)]),
    "frog_jlabels_add": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(FrogVolume), C.POINTER(FrogVolume), C.c_int, C.c_double,
                                   C.c_double, C.POINTER(FrogVolume), C.POINTER(FrogVolume)]),
    "frog_jlabels_finish": (C.c_int, [C.c_void_p, c_u32_p]),
    "frog_jlabels_values": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "frog_jlabels_fused": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(FrogVolume), c_float_p]),
    "frog_jlabels_probability": (C.c_int, [C.c_void_p, C.c_int64, c_float_p]),
    "frog_jlabels_weight": (C.c_int, [C.c_void_p, C.c_uint32, c_float_p]),
    "frog_jlabels_destroy": (None, [C.c_void_p]),
    "frog_distance_map": (C.c_int, [C.POINTER(FrogVolume), C.c_int64, C.c_int, C.c_int, c_u32_p]),
    "frog_surface_create": (C.c_int, [C.POINTER(FrogVolume), C.POINTER(C.c_int64), C.c_uint32, C.c_uint32, C.c_int,
                                      C.POINTER(C.c_void_p)]),
    "frog_surface_add": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(FrogVolume), C.c_double, C.POINTER(FrogSurfaceRow)]),
    "frog_surface_destroy": (None, [C.c_void_p]),
    "frog_isosurface_create": (C.c_int, [C.POINTER(FrogVolume), C.c_int, C.c_double, C.c_int64, C.c_int, C.POINTER(C.c_void_p),
                                         c_u32_p, c_u32_p]),
    "frog_isosurface_apply": (C.c_int, [C.c_void_p, C.c_void_p]),
    "frog_isosurface_get": (C.c_int, [C.c_void_p, c_float_p, c_u32_p]),
    "frog_isosurface_destroy": (None, [C.c_void_p]),
    "frog_chain_apply_f32": (C.c_int, [C.c_void_p, c_float_p, c_float_p, C.c_size_t]),
    "frog_mesh_smooth": (C.c_int, [c_float_p, C.c_size_t, c_u32_p, c_u32_p, C.c_size_t, C.c_uint32, C.c_double, C.c_double, C.c_int,
                                   C.c_int]),
    "frog_isosurface_smooth": (C.c_int, [C.c_void_p, C.c_uint32, C.c_double, C.c_double, C.c_int]),
    "frog_isosurface_upload": (C.c_int, [c_float_p, C.c_uint32, c_u32_p, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]),
    "frog_isosurface_cluster": (C.c_int, [C.c_void_p, C.c_double, c_u32_p, c_u32_p, c_u32_p]),
    "frog_match_options_default": (None, [C.POINTER(FrogMatchOptions)]),
    "frog_matcher_create": (C.c_int, [C.POINTER(FrogKeypoints), C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]),
    "frog_matcher_destroy": (None, [C.c_void_p]),
    "frog_matcher_run": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint16), C.POINTER(C.c_uint16), C.c_size_t,
                                   C.POINTER(FrogMatchOptions), C.POINTER(C.c_uint64), C.POINTER(c_u32_p),
                                   C.POINTER(c_u32_p)]),
    "frog_match_free": (None, [C.c_void_p]),
    "frog_matcher_last_stats": (C.c_int, [C.c_void_p, c_double_p, c_double_p]),
    "frog_matcher_last_forms": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "frog_match_test_products": (C.c_int, [C.c_int, c_float_p, c_float_p, C.c_uint32, C.c_int, c_float_p, c_float_p]),
    "frog_get_points2_subset": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t, c_float_p]),
    "frog_set_hard_links": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_size_t, C.c_float]),
    "frog_residual_sums": (C.c_int, [C.c_void_p]),
    "frog_get_error_map": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(FrogGridInfo), c_float_p, C.c_size_t]),
    "frog_comm_buffer": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                   C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "frog_update_stats_local": (C.c_int, [C.c_void_p]),
    "frog_stats_publish": (C.c_int, [C.c_void_p]),
    "frog_transform_points_local": (C.c_int, [C.c_void_p, C.c_int]),
    "frog_linear_step_local": (C.c_int, [C.c_void_p]),
    "frog_energy_read": (C.c_int, [C.c_void_p, c_double_p, c_double_p]),
    "frog_bounds_local": (C.c_int, [C.c_void_p, c_double_p, c_double_p]),
    "frog_deformable_setup_bounds": (C.c_int, [C.c_void_p, C.c_int, c_double_p, c_double_p, C.POINTER(FrogGridInfo)]),
    "frog_deformable_phase_a": (C.c_int, [C.c_void_p, C.c_float]),
    "frog_deformable_phase_b": (C.c_int, [C.c_void_p]),
    "frog_deformable_phase_c": (C.c_int, [C.c_void_p, c_double_p]),
    "frog_get_stream": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]),
    "frog_comm_unpack_slab": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64), C.c_uint32]),
    "frog_comm_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "frog_create_seconds": (C.c_int, [C.c_void_p, c_double_p, C.POINTER(C.c_int)]),
    "frog_lattice_reallocations": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "frog_transform_points_slab": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_uint32]),
    "frog_comm_unpack_slab_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64), C.c_uint32, C.c_uint32]),
    "frog_step_finish": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "frog_step_speculate": (C.c_int, [C.c_void_p]),
    "frog_cull_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "frog_cull_stats_linear": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "frog_test_stray_points": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "frog_test_scatter_accumulate": (C.c_int, [C.c_int, c_float_p, c_float_p, C.c_size_t, c_float_p, c_float_p, C.c_int]),
    "frog_test_cull_ranges": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "frog_test_cull_steps": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "frog_test_cull_readback": (C.c_int, [C.c_void_p, c_float_p, c_float_p, c_float_p, c_u32_p, c_float_p, c_u32_p]),
    "frog_test_em_refit": (C.c_int, [C.c_void_p, C.c_int]),
    "frog_test_ransac_candidates": (C.c_int, [C.POINTER(FrogModel), C.c_uint32, C.POINTER(FrogRansacOptions), c_double_p,
                                              C.POINTER(C.c_ubyte), C.c_size_t, C.POINTER(C.c_size_t)]),
    "frog_test_ransac_census": (C.c_int, [C.c_void_p, C.POINTER(FrogModel), C.c_uint32, c_double_p, C.c_size_t, C.c_float,
                                          c_u32_p]),
    "frog_test_inlier_probability": (C.c_int, [C.c_int, c_float_p, c_float_p, C.c_size_t, c_float_p, c_float_p]),
    "frog_test_inlier_weight_pair": (C.c_int, [C.c_int, c_float_p, c_float_p, C.c_float, c_float_p, C.c_size_t, c_float_p,
                                              C.POINTER(C.c_ubyte)]),
    "frog_test_bspline_weights": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "frog_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "frog_profile_read": (C.c_int, [C.c_void_p, C.POINTER(FrogKernelTime), C.c_int]),
}

HOST_SYMBOLS = {
    "frog_pairs_read": (C.c_void_p, [C.c_char_p, C.POINTER(C.c_int)]),
    "frog_pairs_write": (C.c_int, [C.c_void_p, C.c_char_p]),
    "frog_pairs_free": (None, [C.c_void_p]),
    "frog_pairs_model": (None, [C.c_void_p, C.POINTER(FrogModel)]),
    "frog_pairs_num_pairs": (C.c_uint64, [C.c_void_p]),
    "frog_pairs_num_points": (C.c_uint64, [C.c_void_p]),
    "frog_pairs_num_images": (C.c_uint32, [C.c_void_p]),
    "frog_pairs_num_blocks": (C.c_uint32, [C.c_void_p]),
    "frog_host_threads": (C.c_int, []),
    "frog_pairs_block": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint16), C.POINTER(C.c_uint16),
                                   C.POINTER(C.c_uint32), C.POINTER(c_u32_p), C.POINTER(c_u32_p)]),
    "frog_pairs_from_arrays": (C.c_void_p, [C.c_uint32, c_u32_p, c_float_p, c_float_p, C.c_uint32,
                                            C.POINTER(C.c_uint16), C.POINTER(C.c_uint16),
                                            C.POINTER(C.c_uint64), c_u32_p, c_u32_p]),
    "frog_synth_defaults": (None, [C.POINTER(FrogSynthParams)]),
    "frog_synth_generate": (C.c_void_p, [C.POINTER(FrogSynthParams)]),
    "frog_pairs_append_points": (C.c_int, [C.c_void_p, C.c_uint32, c_float_p, C.c_uint32]),
    "frog_pairs_set_points": (C.c_int, [C.c_void_p, C.c_uint32, c_float_p]),
    "frog_volume_read": (C.c_void_p, [C.c_char_p, C.POINTER(C.c_int)]),
    "frog_volume_free": (None, [C.c_void_p]),
    "frog_volume_view": (None, [C.c_void_p, C.POINTER(FrogVolume)]),
    "frog_volume_range": (C.c_int, [C.POINTER(FrogVolume), c_double_p, c_double_p]),
    "frog_volume_write": (C.c_int, [C.c_char_p, C.POINTER(FrogVolume)]),
    "frog_bbox_grid": (C.c_int, [C.c_char_p, C.c_double, C.POINTER(FrogVolume)]),
    "frog_score_metrics_from": (C.c_int, [C.POINTER(FrogScoreSums), C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(FrogScoreMetrics)]),
    "frog_keypoints_read": (C.c_void_p, [C.c_char_p, C.POINTER(C.c_int)]),
    "frog_keypoints_free": (None, [C.c_void_p]),
    "frog_keypoints_count": (C.c_uint32, [C.c_void_p]),
    "frog_keypoints_view": (None, [C.c_void_p, C.POINTER(FrogKeypoints)]),
    "frog_keypoints_select": (C.c_int, [C.c_void_p, c_u32_p, C.c_uint32]),
    "frog_keypoints_write": (C.c_int, [C.c_char_p, C.POINTER(FrogKeypoints)]),
    "frog_transform_read": (C.c_void_p, [C.c_char_p, C.POINTER(C.c_int)]),
    "frog_transform_free": (None, [C.c_void_p]),
    "frog_transform_num_links": (C.c_uint32, [C.c_void_p]),
    "frog_transform_links": (C.POINTER(FrogChainLink), [C.c_void_p]),
    "frog_volume_geometry": (C.c_int, [C.c_char_p, C.POINTER(C.c_uint32), c_double_p, c_double_p]),
    "frog_nifti_write": (C.c_int, [C.c_char_p, C.POINTER(C.c_uint32), c_double_p, c_double_p, C.c_uint32, c_float_p]),
    "frog_run_schedule": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(FrogSchedulePlan), C.POINTER(FrogScheduleResult)]),
    "frog_mesh_read": (C.c_void_p, [C.c_char_p, C.POINTER(C.c_int)]),
    "frog_mesh_view": (None, [C.c_void_p, C.POINTER(FrogMesh)]),
    "frog_mesh_free": (None, [C.c_void_p]),
    "frog_mesh_write": (C.c_int, [C.c_char_p, C.POINTER(FrogMesh)]),
    "frog_mesh_last_error": (C.c_char_p, []),
}

# include/frog_comm.h (libfrog_comm.so: RCCL; loaded only by hosts that shard over GPUs from C)
COMM_SYMBOLS = {
    "frog_comm_create_rccl": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_void_p)]),
    "frog_comm_create_loopback": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "frog_comm_unique_id": (C.c_int, [C.POINTER(C.c_ubyte)]),
    "frog_comm_create_rank": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_ubyte), C.c_int, C.POINTER(C.c_void_p)]),
    "frog_comm_create_shm": (C.c_int, [C.c_int, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]),
    "frog_comm_set_rows": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "frog_comm_destroy_all": (None, [C.c_int, C.POINTER(C.c_void_p)]),
    "frog_comm_bind": (C.c_int, [C.c_void_p, C.c_void_p, c_u32_p]),
    "frog_comm_all_gather_xyz2": (C.c_int, [C.c_void_p]),
    "frog_comm_slab": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "frog_comm_all_gather_slab": (C.c_int, [C.c_void_p]),
    "frog_comm_gather_points": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_uint32]),
    "frog_comm_all_reduce": (C.c_int, [C.c_void_p, C.c_int]),
    "frog_comm_all_reduce_bounds": (C.c_int, [C.c_void_p, c_double_p, c_double_p]),
    "frog_comm_barrier": (C.c_int, [C.c_void_p]),
    "frog_comm_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "frog_comm_timing_read": (C.c_int, [C.c_void_p, c_double_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
}


def _load(name, symbols):
    path = os.path.join(LIB_DIR, name)
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"(or `make -C frog_amd/csrc`). frog_amd has no fallback for its native libraries.")
    lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
    for sym, (res, args) in symbols.items():
        fn = getattr(lib, sym)          # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    return lib


_hip = None
_host = None
_comm = None


def comm_lib():
    """libfrog_comm.so (maps RCCL): only for hosts that shard over GPUs through include/frog_comm.h."""
    global _comm
    if _comm is None:
        hip_lib()
        _comm = _load("libfrog_comm.so", COMM_SYMBOLS)
    return _comm


def hip_lib():
    global _hip
    if _hip is None:
        # FROG_HIP_LIB: another build of the SAME library (kernel tuning experiments); relative to lib/
        _hip = _load(os.environ.get("FROG_HIP_LIB", "libfrog_hip.so"), HIP_SYMBOLS)
    return _hip


def host_lib():
    global _host
    if _host is None:
        hip_lib()                       # libfrog_host.so links against it
        _host = _load("libfrog_host.so", HOST_SYMBOLS)
    return _host


class FrogError(RuntimeError):
    def __init__(self, code, where):
        msg = hip_lib().frog_last_error()
        super().__init__(f"{where}: status {code}: {msg.decode() if msg else ''}")
        self.code = code


def check(code, where):
    if code != FROG_OK:
        raise FrogError(code, where)
