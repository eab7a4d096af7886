"""Scalar volumes for the reslicing step (tools/VolumeTransform.cxx): NIfTI-1 and MetaImage files through the
host library's reader and writer (include/frog_host.h)."""
import ctypes as C

import numpy as np

from . import _abi


def read_volume(path):
    """(voxels[z, y, x], origin(x, y, z), spacing(x, y, z)) of a .nii/.nii.gz/.mhd/.mha file."""
    lib = _abi.host_lib()
    status = C.c_int()
    h = lib.frog_volume_read(str(path).encode(), C.byref(status))
    if not h:
        raise OSError(f"cannot read volume {path} (status {status.value})")
    try:
        v = _abi.FrogVolume()
        lib.frog_volume_view(h, C.byref(v))
        dt = np.dtype(_abi.FROG_V_DTYPES[v.dtype])
        n = v.dims[0] * v.dims[1] * v.dims[2]
        buf = (C.c_char * (n * dt.itemsize)).from_address(v.data)
        a = np.frombuffer(buf, dt).reshape(v.dims[2], v.dims[1], v.dims[0]).copy()
        return a, tuple(v.origin), tuple(v.spacing)
    finally:
        lib.frog_volume_free(h)


def write_volume(path, voxels, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0)):
    """voxels[z, y, x] to .mhd (+ .zraw beside it), .nii or .nii.gz."""
    a = np.ascontiguousarray(voxels)
    v = _abi.volume_view(a, origin, spacing)
    rc = _abi.host_lib().frog_volume_write(str(path).encode(), C.byref(v))
    if rc:
        raise OSError(f"cannot write volume {path} (status {rc})")


def bbox_grid(path, spacing):
    """DummyVolumeGenerator's grid over bbox.json's box (frog_bbox_grid): (dims(x, y, z), origin, spacing)."""
    v = _abi.FrogVolume()
    _abi.check(_abi.host_lib().frog_bbox_grid(str(path).encode(), float(spacing), C.byref(v)), "frog_bbox_grid")
    return tuple(v.dims), tuple(v.origin), tuple(v.spacing)


def _as_volume(item):
    """(voxels[z, y, x], origin, spacing) as read_volume returns it, or a bare array (origin 0, spacing 1)."""
    if isinstance(item, np.ndarray):
        return np.ascontiguousarray(item), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    a, o, s = item
    return np.ascontiguousarray(a), tuple(float(v) for v in o), tuple(float(v) for v in s)


class _Accumulator:
    """What Average, CoverAverage and Labels share: the grid (`dims`, `_grid`), the handle `_h` that the library's
    frog_<_NAME>_create gives and its frog_<_NAME>_destroy takes back, and the views an add hands to the library."""

    _NAME = None

    def __init__(self, grid, *create_args):
        self._lib = _abi.hip_lib()
        dims, origin, spacing = grid
        self.dims = tuple(int(d) for d in dims)
        self._grid = _abi.volume_view(None, origin, spacing, self.dims)
        self._h = C.c_void_p()
        where = f"frog_{self._NAME}_create"
        _abi.check(getattr(self._lib, where)(C.byref(self._grid), *create_args, C.byref(self._h)), where)

    def close(self):
        if self._h:
            getattr(self._lib, f"frog_{self._NAME}_destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _views(self, volume, mask=None, resliced=False):
        """(voxels, source, mask, view, out): the source's array; what the library takes as the source, as the mask and as
        the resliced volume, the last a view of the new grid-sized array `out` of the source's type (None where there is no
        mask, or no resliced volume is wanted).  Each reference keeps the array behind it alive."""
        def ref(a, origin, spacing):
            v = _abi.volume_view(a, origin, spacing)
            v.voxels = a                                            # _as_volume may have made a contiguous copy
            return C.byref(v)

        a, o, s = _as_volume(volume)
        out = np.empty(self.dims[::-1], a.dtype) if resliced else None
        return (a, ref(a, o, s), None if mask is None else ref(*_as_volume(mask)),
                ref(out, tuple(self._grid.origin), tuple(self._grid.spacing)) if resliced else None, out)


def _group(volumes, chains, masks, grid):
    """The arguments average(), cover_average(), group_quality() and fuse_labels() share, checked: the volumes as
    (voxels, origin, spacing) and the grid, by default the first volume's."""
    vols = [_as_volume(v) for v in volumes]
    if not vols:
        raise ValueError("no volumes")
    if chains is not None and len(chains) != len(vols):
        raise ValueError("one chain per volume expected")
    if masks is not None and len(masks) != len(vols):
        raise ValueError("one mask per volume expected")
    if grid is None:
        a, o, s = vols[0]
        grid = (a.shape[::-1], o, s)
    return vols, grid


class Average(_Accumulator):
    """frog_average (include/frog_chain.h): n_images volumes added one by one on `grid` = (dims(x, y, z), origin, spacing),
    then the f32 mean and stdev of AverageVolumes.cxx."""

    _NAME = "average"

    def __init__(self, grid, n_images, device=0):
        super().__init__(grid, int(n_images), int(device))

    def add(self, volume, chain=None, interpolation=1, background=0.0, resliced=False):
        """Adds `volume` ((voxels, origin, spacing) or an array already on the grid when chain is None); with a chain
        (frog_amd.chain.Chain, grid space -> volume space) it is resliced first as Chain.reslice does.  resliced=True
        returns that volume (source dtype, shape dims[::-1])."""
        _, src, _, ov, out = self._views(volume, None, resliced)
        _abi.check(self._lib.frog_average_add(self._h, chain._h if chain is not None else None, src, int(interpolation),
                                              float(background), ov), "frog_average_add")
        return out

    def finish(self):
        """(mean, stdev), float32 arrays of shape dims[::-1]."""
        mean = np.empty(self.dims[::-1], np.float32)
        stdev = np.empty_like(mean)
        _abi.check(self._lib.frog_average_finish(self._h, mean.ctypes.data_as(_abi.c_float_p), stdev.ctypes.data_as(_abi.c_float_p)),
                   "frog_average_finish")
        return mean, stdev


def average(volumes, chains=None, grid=None, interpolation=1, backgrounds=None, device=0):
    """Voxel-wise mean and stdev of a group on the device (tools/AverageVolumes.cxx; with `chains`, transform.sh's
    VolumeTransform + AverageVolumes).  `volumes`: (voxels[z, y, x], origin, spacing) tuples or arrays; `chains`: None (the
    volumes are on the grid already) or one frog_amd.chain.Chain per volume, mapping grid space to the volume's;
    `grid`: (dims(x, y, z), origin, spacing), default the first volume's; `backgrounds`: None (each volume's minimum, as
    VolumeTransform), a number or one per volume.  Returns float32 (mean, stdev), NaN where upstream's f32 variance
    rounds negative."""
    vols, grid = _group(volumes, chains, None, grid)
    if backgrounds is None:
        backgrounds = [float(a.min()) for a, _, _ in vols]
    elif np.ndim(backgrounds) == 0:
        backgrounds = [float(backgrounds)] * len(vols)
    acc = Average(grid, len(vols), device)
    try:
        for k, v in enumerate(vols):
            acc.add(v, None if chains is None else chains[k], interpolation, backgrounds[k])
        return acc.finish()
    finally:
        acc.close()


class CoverAverage(_Accumulator):
    """frog_cover (include/frog_chain.h): volumes added one by one on `grid` = (dims(x, y, z), origin, spacing), each only
    where it covers the voxel (and its mask is non-zero); then the f32 mean and stdev over the covering images and their
    count."""

    _NAME = "cover"

    def __init__(self, grid, device=0):
        super().__init__(grid, int(device))

    def add(self, volume, chain=None, mask=None, interpolation=1, background=0.0, resliced=False):
        """Adds `volume` ((voxels, origin, spacing) or an array already on the grid when chain is None) where it is valid:
        with a chain (frog_amd.chain.Chain, grid space -> volume space) where the sample lies inside the volume as
        Chain.reslice decides it, without one everywhere; and, with `mask` (an integer volume of its own geometry, given
        like `volume`), where the mask's nearest voxel is non-zero.  resliced=True returns the volume Chain.reslice would
        give with `background` (source dtype, shape dims[::-1])."""
        _, src, mv, ov, out = self._views(volume, mask, resliced)
        _abi.check(self._lib.frog_cover_add(self._h, chain._h if chain is not None else None, src, mv, int(interpolation),
                                            float(background), ov), "frog_cover_add")
        return out

    def finish(self, min_count=1, fill=0.0):
        """(mean, stdev, count): float32, float32 and uint16 arrays of shape dims[::-1]; where fewer than min_count images
        were valid the mean is `fill` and the stdev 0.  May be called again, and after further adds."""
        mean = np.empty(self.dims[::-1], np.float32)
        stdev = np.empty_like(mean)
        count = np.empty(self.dims[::-1], np.uint16)
        _abi.check(self._lib.frog_cover_finish(self._h, int(min_count), float(fill), mean.ctypes.data_as(_abi.c_float_p),
                                               stdev.ctypes.data_as(_abi.c_float_p), count.ctypes.data_as(C.POINTER(C.c_uint16))),
                   "frog_cover_finish")
        return mean, stdev, count

    def score(self, volume, chain=None, mask=None, interpolation=1, background=None, min_count=1, leave_one_out=True, bins=64,
              value_range=None):
        """One image against the accumulator's mean (frog_cover_score), over the voxels where add() with the same `volume`,
        `chain`, `mask` and `interpolation` counts it and at least max(2 if leave_one_out else 1, min_count) images do.
        leave_one_out: the image is one of the adds and is taken out of the mean again; False for an image that is not.
        `background` (default the volume's minimum) never enters a sum.  bins=0: no histogram; else `value_range` = (lo, hi)
        of the bins x bins joint histogram (row = the image's bin), default quality_range(min_count).  Returns a dict: the
        sums n, n_nonfinite, sx, sy, sxx, syy, sxy, sad; covered_fraction = n / grid voxels; `histogram` (uint64, (bins,
        bins)) or None; and ncc, mean_abs_diff, rmse, mi, nmi from frog_score_metrics_from.  Leaves the accumulator as it is."""
        a, src, mv, _, _ = self._views(volume, mask)
        if background is None:
            background = float(a.min())
        bins = int(bins)
        hist, lo, hi = None, 0.0, 0.0
        if bins:
            lo, hi = self.quality_range(min_count) if value_range is None else value_range
            hist = np.zeros((bins, bins), np.uint64)
        hist_p = hist.ctypes.data_as(C.POINTER(C.c_uint64)) if hist is not None else None
        sums = _abi.FrogScoreSums()
        _abi.check(self._lib.frog_cover_score(self._h, chain._h if chain is not None else None, src, mv, int(interpolation),
                                              float(background), int(min_count), int(bool(leave_one_out)), bins, float(lo),
                                              float(hi), C.byref(sums), hist_p), "frog_cover_score")
        metrics = _abi.FrogScoreMetrics()
        _abi.check(_abi.host_lib().frog_score_metrics_from(C.byref(sums), hist_p, bins, C.byref(metrics)), "frog_score_metrics_from")
        out = {name: getattr(sums, name) for name, _ in sums._fields_}
        out["covered_fraction"] = sums.n / float(np.prod(self.dims))
        out["histogram"] = hist
        out.update({name: getattr(metrics, name) for name, _ in metrics._fields_})
        return out

    def quality_range(self, min_count=1):
        """The default histogram range of score(), and of bin/AverageImage -q 1: (lo, hi) = the smallest finite value of the
        mean over the voxels with count >= min_count, and the float32 after the largest."""
        mean, _, count = self.finish(min_count)
        v = mean[(count >= min_count) & np.isfinite(mean)]
        if not v.size:
            raise ValueError("no voxel with a finite mean and at least min_count images")
        return float(v.min()), float(np.nextafter(v.max(), np.float32(np.inf)))


def cover_average(volumes, chains=None, masks=None, grid=None, interpolation=1, min_count=1, fill=0.0, device=0):
    """Voxel-wise mean, stdev and count over the images that cover each grid voxel (bin/AverageImage -c 1).  `volumes`,
    `chains` and `grid` as in average(); `masks`: None or one integer volume (or None) per image.  Returns
    (mean float32, stdev float32, count uint16)."""
    vols, grid = _group(volumes, chains, masks, grid)
    acc = CoverAverage(grid, device)
    try:
        for k, v in enumerate(vols):
            acc.add(v, None if chains is None else chains[k], None if masks is None else masks[k], interpolation)
        return acc.finish(min_count, fill)
    finally:
        acc.close()


def robust_z(values):
    """(v - median) / (1.4826 MAD) over the finite entries, in float64; 0 everywhere where the MAD is 0, NaN where v is not
    finite.  The median of an even number is the mean of the middle two."""
    v = np.asarray(values, np.float64)
    finite = np.isfinite(v)
    z = np.full(v.shape, np.nan)
    if finite.any():
        median = _median(v[finite])
        mad = _median(np.abs(v[finite] - median))
        z[finite] = (v[finite] - median) / (1.4826 * mad) if mad > 0 else 0.0
    return z


def _median(v):
    s = np.sort(v)
    n = len(s)
    return s[n // 2] if n % 2 else (s[n // 2 - 1] + s[n // 2]) / 2.0


def group_quality(volumes, chains=None, masks=None, grid=None, interpolation=1, min_count=1, bins=64, value_range=None, device=0):
    """Which images of a registered group registered badly (bin/AverageImage -c 1 -q 1): the coverage-aware average of the
    group, then every image against the mean of the others over the voxels it covers (CoverAverage.score with
    leave_one_out).  Arguments as in cover_average(); the background of image k is its minimum.  Returns one dict per image,
    score()'s plus `image` (its index) and `ncc_robust_z` (robust_z of the group's ncc): a low ncc or nmi, and a strongly
    negative z, single out an image that does not match the rest."""
    vols, grid = _group(volumes, chains, masks, grid)
    acc = CoverAverage(grid, device)
    try:
        for k, v in enumerate(vols):
            acc.add(v, None if chains is None else chains[k], None if masks is None else masks[k], interpolation)
        if bins and value_range is None:
            value_range = acc.quality_range(min_count)
        rows = []
        for k, v in enumerate(vols):
            row = acc.score(v, None if chains is None else chains[k], None if masks is None else masks[k], interpolation, None,
                            min_count, True, bins, value_range)
            row["image"] = k
            rows.append(row)
    finally:
        acc.close()
    for row, z in zip(rows, robust_z([r["ncc"] for r in rows])):
        row["ncc_robust_z"] = float(z)
    return rows


class RankImages(_Accumulator):
    """frog_rank (include/frog_chain.h): every added image's value per voxel of a window of `grid` = (dims(x, y, z), origin,
    spacing), then per-voxel order statistics over the images that take part: quantile images, the MAD and the count.
    `window` = (first z-plane, planes), default the whole grid; `n_images` is the most adds it will take."""

    _NAME = "rank"

    def __init__(self, grid, n_images, window=None, device=0):
        first, planes = (0, int(grid[0][2])) if window is None else (int(window[0]), int(window[1]))
        super().__init__(grid, first, planes, int(n_images), int(device))
        self.window = (first, planes)
        self.shape = (planes,) + self.dims[1::-1]

    def add(self, volume, chain=None, mask=None, interpolation=1, background=0.0):
        """Keeps `volume` where CoverAverage.add with the same arguments would count it and its value is not NaN."""
        _, src, mv, _, _ = self._views(volume, mask)
        _abi.check(self._lib.frog_rank_add(self._h, chain._h if chain is not None else None, src, mv, int(interpolation),
                                           float(background)), "frog_rank_add")

    def finish(self, min_count=1, fill=0.0, quantiles=(0.5,), mad=True, count=True):
        """(values, mad, count) over the window: `values` float32 of shape (len(quantiles),) + shape, one image per
        probability (linear interpolation between the two neighbouring order statistics); `mad` the raw median absolute
        deviation, float32, or None; `count` uint16, the images that took part, or None.  Where fewer than min_count did,
        the values are `fill` and the MAD 0.  May be called again, and after further adds."""
        q = np.ascontiguousarray(quantiles, np.float64).ravel()
        values = np.empty((len(q),) + self.shape, np.float32)
        m = np.empty(self.shape, np.float32) if mad else None
        c = np.empty(self.shape, np.uint16) if count else None
        _abi.check(self._lib.frog_rank_finish(self._h, int(min_count), float(fill), len(q), q.ctypes.data_as(C.POINTER(C.c_double)),
                                              values.ctypes.data_as(_abi.c_float_p) if len(q) else None,
                                              m.ctypes.data_as(_abi.c_float_p) if mad else None,
                                              c.ctypes.data_as(C.POINTER(C.c_uint16)) if count else None), "frog_rank_finish")
        return values, m, c


def rank_planes(grid, n_images, device=0):
    """The most z-planes of `grid` a RankImages window for n_images may hold on the device now (frog_rank_planes)."""
    dims, origin, spacing = grid
    g = _abi.volume_view(None, origin, spacing, tuple(int(d) for d in dims))
    planes = C.c_uint32()
    _abi.check(_abi.hip_lib().frog_rank_planes(C.byref(g), int(n_images), int(device), C.byref(planes)), "frog_rank_planes")
    return planes.value


def group_median(volumes, chains=None, masks=None, grid=None, quantiles=(), interpolation=1, min_count=1, fill=0.0, max_planes=None,
                 device=0):
    """The robust atlas of a registered group (bin/AverageImage -c 1 -r 1): per grid voxel the median, the raw MAD (x 1.4826
    for a normal stdev) and the count of the images that cover it, and one image per probability in `quantiles`.  Arguments as
    in cover_average(); the device holds slabs of rank_planes() z-planes (at most max_planes) and the images are added once
    per slab, which changes no bit.  Returns (median float32, mad float32, count uint16, {q: float32 image})."""
    vols, grid = _group(volumes, chains, masks, grid)
    qs = [float(q) for q in quantiles]
    dims = tuple(int(d) for d in grid[0])
    planes = rank_planes(grid, len(vols), device)
    if max_planes is not None:
        planes = max(1, min(planes, int(max_planes)))
    values = np.empty((1 + len(qs),) + dims[::-1], np.float32)
    mad = np.empty(dims[::-1], np.float32)
    count = np.empty(dims[::-1], np.uint16)
    for first in range(0, dims[2], planes):
        n = min(planes, dims[2] - first)
        acc = RankImages(grid, len(vols), (first, n), device)
        try:
            for k, v in enumerate(vols):
                acc.add(v, None if chains is None else chains[k], None if masks is None else masks[k], interpolation)
            values[:, first:first + n], mad[first:first + n], count[first:first + n] = acc.finish(min_count, fill, [0.5] + qs)
        finally:
            acc.close()
    return values[0], mad, count, {q: values[1 + j] for j, q in enumerate(qs)}


class GroupGLM(_Accumulator):
    """frog_glm (include/frog_chain.h): every added image's value per voxel of a window of `grid`, then per voxel the linear
    model of those values on `design` (n_images x n_columns, row i belongs to add number i) over the images that take part
    there: coefficients, residual stdev, one t per contrast, and the extrema of t under permutations of the design.
    `window` = (first z-plane, planes), default the whole grid."""

    _NAME = "glm"

    def __init__(self, grid, design, window=None, device=0, smooth=0.0):
        X = np.ascontiguousarray(design, np.float64)
        if X.ndim != 2:
            raise ValueError("design: one row per image, one column per regressor")
        first, planes = (0, int(grid[0][2])) if window is None else (int(window[0]), int(window[1]))
        super().__init__(grid, first, planes, X.shape[0], X.shape[1], X.ctypes.data_as(_abi.c_double_p), int(device))
        self.design = X
        self.window = (first, planes)
        self.shape = (planes,) + self.dims[1::-1]
        if smooth:
            try:
                self.smooth(smooth)
            except Exception:
                self.close()
                raise

    def smooth(self, sigma):
        """Before the first add: every add from now on stores its map smoothed by the coverage-aware Gaussian of `sigma` mm
        (smooth_volume() of the whole-grid map, of which the window's part is kept); 0 turns it off (frog_glm_smooth)."""
        _abi.check(self._lib.frog_glm_smooth(self._h, float(sigma)), "frog_glm_smooth")

    def add(self, volume, chain=None, mask=None, interpolation=1, background=0.0):
        """Keeps `volume` where CoverAverage.add with the same arguments would count it and its value is finite."""
        _, src, mv, _, _ = self._views(volume, mask)
        _abi.check(self._lib.frog_glm_add(self._h, chain._h if chain is not None else None, src, mv, int(interpolation),
                                          float(background)), "frog_glm_add")

    def add_jacobian(self, chain, support=None, mask=None, log=True):
        """Keeps the Jacobian determinant of `chain` at every window voxel (what Chain.sample gives there), or with `log` its
        logarithm where it is positive.  `support` = (dims(x, y, z), origin, spacing): the voxel counts only where the chain
        takes it inside that geometry; `mask` as in add."""
        sv = None
        if support is not None:
            dims, origin, spacing = support
            sv = C.byref(_abi.volume_view(None, tuple(float(v) for v in origin), tuple(float(v) for v in spacing), tuple(int(d) for d in dims)))
        mv = self._views(mask)[1] if mask is not None else None
        _abi.check(self._lib.frog_glm_add_jacobian(self._h, chain._h if chain is not None else None, sv, mv, int(bool(log))),
                   "frog_glm_add_jacobian")

    def plane(self, image_index):
        """What add number image_index stored over the window: float32, NaN (0x7FC00000) where it does not take part."""
        out = np.empty(self.shape, np.float32)
        _abi.check(self._lib.frog_glm_plane(self._h, int(image_index), out.ctypes.data_as(_abi.c_float_p)), "frog_glm_plane")
        return out

    def _fit_arguments(self, contrasts, region):
        c = np.ascontiguousarray(contrasts, np.float64).reshape(-1, self.design.shape[1])
        r = None if region is None else np.ascontiguousarray(np.asarray(region) != 0, np.uint8)
        if r is not None and r.shape != self.shape:
            raise ValueError("region: one value per window voxel")
        return c, r, None if r is None else r.ctypes.data_as(C.POINTER(C.c_uint8))

    def finish(self, contrasts, min_count=1, sigma_floor=0.0, region=None, fill=0.0):
        """(beta, sigma, t, count) over the window: beta float32 (n_columns,) + shape, sigma float32, t float32 (n_contrasts,)
        + shape, count uint16.  Voxels that are not fit hold `fill` in beta, sigma and t; a fit voxel whose residual stdev is
        <= sigma_floor has t = NaN."""
        c, _r, rp = self._fit_arguments(contrasts, region)
        beta = np.empty((self.design.shape[1],) + self.shape, np.float32)
        sigma = np.empty(self.shape, np.float32)
        t = np.empty((len(c),) + self.shape, np.float32)
        count = np.empty(self.shape, np.uint16)
        _abi.check(self._lib.frog_glm_finish(self._h, len(c), c.ctypes.data_as(_abi.c_double_p), int(min_count), float(sigma_floor), rp,
                                             float(fill), beta.ctypes.data_as(_abi.c_float_p), sigma.ctypes.data_as(_abi.c_float_p),
                                             t.ctypes.data_as(_abi.c_float_p) if len(c) else None,
                                             count.ctypes.data_as(C.POINTER(C.c_uint16))), "frog_glm_finish")
        return beta, sigma, t, count

    def permute(self, contrasts, perm, sign=None, columns=None, min_count=1, sigma_floor=0.0, region=None):
        """(max_t, min_t), float32 (n_perms, n_contrasts): the extrema of each contrast's t over the window's fit voxels under
        every row of `perm` (n_perms x n_images image indices) and `sign` (+-1, or None).  `columns`: the design columns that
        move, an iterable of indices or a bit mask; default all."""
        return self._permute(None, 0, contrasts, perm, sign, columns, min_count, sigma_floor, region)

    def permute_clusters(self, sink, contrasts, perm, sign=None, columns=None, min_count=1, sigma_floor=0.0, region=None, first_perm=0):
        """permute(), which also sets in the ClusterSink `sink`, for row k in the slots of its permutation first_perm + k, the
        bit of every window voxel whose t counts towards the extrema and lies beyond the sink's threshold."""
        return self._permute(sink, first_perm, contrasts, perm, sign, columns, min_count, sigma_floor, region)

    def permute_tfce(self, sink, contrasts, perm, sign=None, columns=None, min_count=1, sigma_floor=0.0, region=None, first_perm=0):
        """permute(), which also stores in the TfceSink `sink`, for row k in the slots of its permutation first_perm + k, the
        level of every window voxel whose t counts towards the extrema, and 0 for the window's other voxels."""
        return self._permute(sink, first_perm, contrasts, perm, sign, columns, min_count, sigma_floor, region)

    def _permute(self, sink, first_perm, contrasts, perm, sign, columns, min_count, sigma_floor, region):
        c, _r, rp = self._fit_arguments(contrasts, region)
        pm = np.ascontiguousarray(perm, np.uint32).reshape(-1, self.design.shape[0])
        sg = None if sign is None else np.ascontiguousarray(sign, np.int8).reshape(pm.shape)
        p = self.design.shape[1]
        bits = (1 << p) - 1 if columns is None else (int(columns) if np.isscalar(columns) else sum(1 << int(j) for j in set(columns)))
        hi = np.empty((len(pm), len(c)), np.float32)
        lo = np.empty((len(pm), len(c)), np.float32)
        shared = (self._h, len(c), c.ctypes.data_as(_abi.c_double_p), int(min_count), float(sigma_floor), rp, bits, len(pm),
                  pm.ctypes.data_as(_abi.c_u32_p), None if sg is None else sg.ctypes.data_as(C.POINTER(C.c_int8)))
        out = (hi.ctypes.data_as(_abi.c_float_p), lo.ctypes.data_as(_abi.c_float_p))
        if sink is None:
            _abi.check(self._lib.frog_glm_permute(*shared, *out), "frog_glm_permute")
        else:
            where = f"frog_glm_permute_{sink._NAME}"
            _abi.check(getattr(self._lib, where)(*shared, int(first_perm), sink._h, *out), where)
        return hi, lo


class _PermutationSink(_Accumulator):
    """What ClusterSink and TfceSink share: the slots (n_perms, n_contrasts, sides) for the whole grid of `shape`, which every
    create takes first, the per-slot value of finish() and a slot's outputs on the grid."""

    def __init__(self, grid, n_perms, n_contrasts, two_sided, *create_args):
        super().__init__(grid, int(n_perms), int(n_contrasts), int(bool(two_sided)), *create_args)
        self.n_perms, self.n_contrasts, self.sides = int(n_perms), int(n_contrasts), 2 if two_sided else 1
        self.shape = self.dims[::-1]

    def _output(self, name, shape, dtype, *slot, extra=()):
        """The new array that frog_<_NAME>_<name>(handle, *slot, the array, *extra) fills."""
        out = np.empty(shape, dtype)
        where = f"frog_{self._NAME}_{name}"
        pointer = out.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(out.dtype)))
        _abi.check(getattr(self._lib, where)(self._h, *slot, pointer, *extra), where)
        return out

    def _finish(self, dtype):
        return self._output("finish", (self.n_perms, self.n_contrasts, self.sides), dtype)

    def _slot(self, name, dtype, perm, contrast, side, *extra):
        """One slot's output `name` on the grid; `extra`: the byref arguments the library's function takes after it."""
        return self._output(name, self.shape, dtype, int(perm), int(contrast), int(side), extra=extra)


class ClusterSink(_PermutationSink):
    """frog_clusters (include/frog_chain.h): on the device, for the whole `grid`, one bit mask per slot (permutation, contrast,
    side) of the voxels whose t lies beyond `threshold` (side 0: t > threshold; with two_sided side 1: t < -threshold), which
    GroupGLM.permute_clusters fills window by window, and the connected components of each mask at `connectivity`."""

    _NAME = "clusters"

    def __init__(self, grid, n_perms, n_contrasts, threshold, two_sided=False, connectivity=26, device=0):
        super().__init__(grid, n_perms, n_contrasts, two_sided, float(threshold), int(connectivity), int(device))

    def finish(self):
        """The largest extent of every slot's mask, uint32 (n_perms, n_contrasts, sides); 0 where no voxel is set."""
        return self._finish(np.uint32)

    def mask(self, perm, contrast, side=0):
        """One slot's mask, bool on the grid."""
        return self._slot("mask", np.uint8, perm, contrast, side) != 0

    def labels(self, perm, contrast, side=0):
        """(labels uint32 on the grid, n): one slot's components numbered 1..n in ascending order of their smallest voxel index."""
        n = C.c_uint32()
        return self._slot("labels", np.uint32, perm, contrast, side, C.byref(n)), n.value


class TfceSink(_PermutationSink):
    """frog_tfce (include/frog_chain.h): on the device, for the whole `grid`, one u8 level per voxel and slot (permutation,
    contrast, side) -- trunc(t / dh) on side 0 and, with two_sided, trunc(-t / dh) on side 1, saturated at 255 -- which
    GroupGLM.permute_tfce fills window by window, and the threshold-free cluster enhancement of each slot with the exponents
    `e` (0.5 or 1, of the extent) and `h` (1 or 2, of the height) at `connectivity`."""

    _NAME = "tfce"

    def __init__(self, grid, n_perms, n_contrasts, dh=0.1, e=0.5, h=2, two_sided=False, connectivity=26, device=0):
        super().__init__(grid, n_perms, n_contrasts, two_sided, float(dh), float(e), float(h), int(connectivity), int(device))

    def finish(self):
        """The largest tfce of every slot, float32 (n_perms, n_contrasts, sides); 0 where no voxel has a positive level."""
        return self._finish(np.float32)

    def levels(self, perm, contrast, side=0):
        """One slot's levels, uint8 on the grid."""
        return self._slot("levels", np.uint8, perm, contrast, side)

    def map(self, perm, contrast, side=0):
        """One slot's enhanced map, float32 on the grid."""
        return self._slot("map", np.float32, perm, contrast, side)


def _null_p(values, null, dtype):
    """The family-wise corrected p of `values` against one contrast's null row: (float32)((1 + #{k >= 1: null[k] >= value}) /
    (double)n_perms).  null[0] belongs to the unpermuted design and is no part of the null; the sort and the comparisons are
    made in `dtype`."""
    ranked = np.sort(np.asarray(null, dtype)[1:])
    beyond = len(ranked) - np.searchsorted(ranked, np.asarray(values, dtype), side="left")
    return ((1 + beyond).astype(np.float64) / np.float64(len(ranked) + 1)).astype(np.float32)


def tfce(stat, dh=0.1, e=0.5, h=2, connectivity=26, side=0, device=0):
    """(tfce float32 on the grid, its maximum) of the float32 array stat[z, y, x] (frog_tfce_volume): the threshold-free
    cluster enhancement of stat (side 0) or of -stat (side 1) in steps of dh, saturated at 255 * dh."""
    a = np.ascontiguousarray(stat)
    v = _abi.volume_view(a, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    out = np.empty(a.shape, np.float32)
    top = C.c_float()
    _abi.check(_abi.hip_lib().frog_tfce_volume(C.byref(v), int(side), float(dh), float(e), float(h), int(connectivity), int(device),
                                               out.ctypes.data_as(_abi.c_float_p), C.byref(top)), "frog_tfce_volume")
    return out, np.float32(top.value)


def tfce_p(tfce, null):
    """The family-wise corrected p of enhanced values: (float32)((1 + #{k >= 1: null[k] >= tfce}) / (double)n_perms), null the
    n_perms largest enhanced values with row 0 the unpermuted design; 1 where tfce == 0.  Signed maps go by magnitude."""
    t = np.abs(np.asarray(tfce, np.float32))
    return np.where(t == 0, np.float32(1), _null_p(t, null, np.float32))


def components(mask, connectivity=26, device=0, largest=False):
    """(labels, n) of the non-zero voxels of the integer array mask[z, y, x] (frog_components): labels uint32, 1..n in ascending
    order of each component's smallest voxel index (scipy.ndimage.label's numbering), 0 elsewhere.  connectivity 6 (faces), 18
    (faces and edges) or 26.  With `largest` also the largest component's voxels: (labels, n, largest)."""
    a = np.ascontiguousarray(mask)
    if a.dtype == bool:
        a = a.view(np.uint8)
    v = _abi.volume_view(a, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    out = np.empty(a.shape, np.uint32)
    n, big = C.c_uint32(), C.c_uint64()
    _abi.check(_abi.hip_lib().frog_components(C.byref(v), int(connectivity), int(device), out.ctypes.data_as(_abi.c_u32_p), C.byref(n), C.byref(big)),
               "frog_components")
    return (out, n.value, big.value) if largest else (out, n.value)


def cluster_p(extent, max_extent):
    """The family-wise corrected p of clusters of `extent` voxels: (float32)((1 + #{k >= 1: max_extent[k] >= extent}) /
    (double)n_perms), max_extent the n_perms largest null extents with row 0 the unpermuted design."""
    return _null_p(extent, max_extent, np.int64)


def glm_planes(grid, n_images, device=0, smooth=0.0):
    """The most z-planes of `grid` a GroupGLM window for n_images may hold on the device now (frog_glm_planes); with `smooth`
    (sigma in mm) together with the scratch of the window's halo (frog_glm_smooth_planes)."""
    dims, origin, spacing = grid
    g = _abi.volume_view(None, origin, spacing, tuple(int(d) for d in dims))
    planes = C.c_uint32()
    if smooth:
        _abi.check(_abi.hip_lib().frog_glm_smooth_planes(C.byref(g), int(n_images), float(smooth), int(device), C.byref(planes)),
                   "frog_glm_smooth_planes")
    else:
        _abi.check(_abi.hip_lib().frog_glm_planes(C.byref(g), int(n_images), int(device), C.byref(planes)), "frog_glm_planes")
    return planes.value


SMOOTH_FWHM = _abi.FROG_SMOOTH_FWHM         # fwhm = SMOOTH_FWHM * sigma (2 sqrt(2 ln 2))


def smooth_taps(sigma, spacing):
    """(radius, taps float64 (radius + 1,)) of one axis of the Gaussian of `sigma` mm at `spacing` mm (frog_smooth_taps):
    radius = ceil(3 sigma / spacing), taps[d] = exp(-(d spacing)^2 / (2 sigma^2)), taps[0] == 1.  Host code: no device is
    needed.  The device uses exactly these doubles."""
    radius = C.c_uint32()
    taps = np.zeros(_abi.FROG_SMOOTH_MAX_RADIUS + 1, np.float64)
    _abi.check(_abi.hip_lib().frog_smooth_taps(float(sigma), float(spacing), C.byref(radius), taps.ctypes.data_as(_abi.c_double_p)),
               "frog_smooth_taps")
    return radius.value, taps[:radius.value + 1].copy()


def smooth_volume(volume, sigma, take=None, spacing=(1.0, 1.0, 1.0), device=0):
    """The float32 array volume[z, y, x] smoothed by the coverage-aware Gaussian of `sigma` mm (frog_smooth_volume): the
    normalised convolution over the voxels that take part -- those with a finite value and, with `take`, a non-zero flag --
    with `spacing` = (x, y, z) in mm.  float32; NaN (0x7FC00000) where the voxel does not take part.  fwhm = SMOOTH_FWHM *
    sigma."""
    a = np.ascontiguousarray(volume)
    v = _abi.volume_view(a, (0.0, 0.0, 0.0), tuple(float(s) for s in spacing))
    flags = None if take is None else np.ascontiguousarray(np.asarray(take) != 0, np.uint8)
    if flags is not None and flags.shape != a.shape:
        raise ValueError("take: one flag per voxel")
    out = np.empty(a.shape, np.float32)
    _abi.check(_abi.hip_lib().frog_smooth_volume(C.byref(v), None if flags is None else flags.ctypes.data_as(C.POINTER(C.c_uint8)), float(sigma),
                                                 int(device), out.ctypes.data_as(_abi.c_float_p)), "frog_smooth_volume")
    return out


def glm_draw(n, n_perms, seed=0, shuffle=True, flip=False):
    """(perm uint32, sign int8), both (n_perms, n): frog_glm_draw's permutations and signs.  Row 0 is the identity with every
    sign +1.  Host code: no device is needed."""
    perm = np.empty((int(n_perms), int(n)), np.uint32)
    sign = np.empty((int(n_perms), int(n)), np.int8)
    _abi.check(_abi.hip_lib().frog_glm_draw(int(n), int(n_perms), int(seed) & (2 ** 64 - 1), int(bool(shuffle)), int(bool(flip)),
                                            perm.ctypes.data_as(_abi.c_u32_p), sign.ctypes.data_as(C.POINTER(C.c_int8))), "frog_glm_draw")
    return perm, sign


def _float_keys(x):
    """frog_rank's keys of float32 values: their unsigned order is -inf < ... < -0 < +0 < ... < +inf."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(u >> 31 != 0, ~u, u ^ np.uint32(0x80000000))


def fwe_p(t, max_t, min_t=None, fit=None):
    """The family-wise corrected p-map of one contrast: p[v] = (float32)((1 + #{k >= 1: max_t[k] >= t[v]}) / (double)n_perms),
    max_t the n_perms maxima over the whole grid with row 0 the unpermuted design.  With min_t the two-sided form: max(max_t,
    -min_t) against |t|.  Voxels outside `fit`, and NaN voxels, get 1."""
    t = np.asarray(t, np.float32)
    hi = np.asarray(max_t, np.float32)
    if min_t is not None:
        hi, t = np.maximum(hi, -np.asarray(min_t, np.float32)), np.abs(t)
    bad = np.isnan(t) if fit is None else (np.isnan(t) | ~np.asarray(fit, bool))
    return np.where(bad, np.float32(1), _null_p(t, hi, np.float32))


def group_glm(design, contrasts, volumes=None, chains=None, masks=None, grid=None, value="logjacobian", supports=None, interpolation=1,
              min_count=1, sigma_floor=0.0, region=None, fill=0.0, n_perms=0, seed=0, columns=None, flip=False, two_sided=False,
              max_planes=None, device=0, cluster_threshold=None, connectivity=26, tfce=False, smooth=0.0):
    """The per-voxel linear model of a registered group (bin/GroupStats).  value "logjacobian" or "jacobian": image i is the
    (log) Jacobian determinant of chains[i] on `grid`, counted where the chain lands inside supports[i] (a geometry, optional)
    and masks[i]; value "images": volumes[i] resliced as in cover_average().  With n_perms > 0 the columns `columns` (default
    those with a non-zero entry in any contrast) are permuted (and with `flip` sign-flipped) n_perms - 1 times by glm_draw(seed),
    row 0 being the design itself.  The device holds slabs of glm_planes() z-planes (at most max_planes); the slabs' extrema are
    combined with max and min, which changes no bit.  Returns a dict: beta, sigma, t, count, fit (bool: the voxel was fit), and
    with permutations max_t, min_t (n_perms, n_contrasts) and p (n_contrasts,) + shape from fwe_p().
    With cluster_threshold and permutations also the cluster-extent test at `connectivity`: one ClusterSink for the whole grid,
    filled by every slab.  max_extent uint32 (n_perms, n_contrasts): the largest cluster of t > cluster_threshold under each
    permutation, with two_sided the larger of that and the largest cluster of t < -cluster_threshold.  clusters int32
    (n_contrasts,) + shape: the observed map's clusters 1..K, with two_sided the negative side's numbered after the positive
    side's.  cluster_extent: per contrast the K extents, uint32.  cluster_p float32 (n_contrasts,) + shape: cluster_p() of the
    voxel's cluster against max_extent, 1 outside every cluster.
    With tfce (True, or a dict of dh, e, h, connectivity in place of 0.1, 0.5, 2 and `connectivity`) and permutations also
    threshold-free cluster enhancement: one TfceSink for the whole grid, filled by every slab with a permute call of its own.
    max_tfce float32 (n_perms, n_contrasts): the largest enhanced value under each permutation, with two_sided the larger of
    the two sides'.  tfce float32 (n_contrasts,) + shape: the observed enhanced map, with two_sided +tfce of the positive side
    and -tfce of the negative.  tfce_p float32: tfce_p() of the map against max_tfce.
    With smooth (sigma in mm; fwhm = SMOOTH_FWHM * sigma = 2.3548... * sigma) every image's map is smoothed before the fit by
    the coverage-aware Gaussian of smooth_volume(), over the voxels at which the image takes part; the slabs are then those of
    glm_planes(smooth=...), which leave room for the scratch of a slab's halo, and still change no bit."""
    X = np.ascontiguousarray(design, np.float64)
    c = np.ascontiguousarray(contrasts, np.float64).reshape(-1, X.shape[1])
    n = X.shape[0]
    images = value == "images"
    if value not in ("logjacobian", "jacobian", "images"):
        raise ValueError("value: logjacobian, jacobian or images")
    if images:
        vols, grid = _group(volumes, chains, masks, grid)
        if len(vols) != n:
            raise ValueError("one design row per volume expected")
    elif chains is None or len(chains) != n or grid is None:
        raise ValueError("a grid and one chain per design row expected")
    dims = tuple(int(d) for d in grid[0])
    shape = dims[::-1]
    reg = None if region is None else np.asarray(region) != 0
    planes = glm_planes(grid, n, device, smooth)
    if max_planes is not None:
        planes = max(1, min(planes, int(max_planes)))
    if columns is None:
        columns = [j for j in range(X.shape[1]) if (c[:, j] != 0).any()]
    out = dict(beta=np.empty((X.shape[1],) + shape, np.float32), sigma=np.empty(shape, np.float32), t=np.empty((len(c),) + shape, np.float32),
               count=np.empty(shape, np.uint16), fit=np.empty(shape, bool))
    draws = glm_draw(n, n_perms, seed, True, flip) if n_perms else None
    sink = ClusterSink(grid, n_perms, len(c), cluster_threshold, two_sided, connectivity, device) if n_perms and cluster_threshold is not None else None
    enhance = None
    if n_perms and tfce:
        opt = dict(dh=0.1, e=0.5, h=2, connectivity=connectivity)
        opt.update(tfce if isinstance(tfce, dict) else {})
        enhance = TfceSink(grid, n_perms, len(c), opt["dh"], opt["e"], opt["h"], two_sided, opt["connectivity"], device)

    def add(acc, k):
        mask = None if masks is None else masks[k]
        if images:
            acc.add(vols[k], None if chains is None else chains[k], mask, interpolation)
        else:
            acc.add_jacobian(chains[k], None if supports is None else supports[k], mask, value == "logjacobian")

    moves = (draws[0], draws[1] if flip else None, columns) if n_perms else None
    hi, lo = _glm_slabs(out, grid, X, c, planes, add, reg, (min_count, sigma_floor, fill), device, smooth, moves, sink, enhance)
    if n_perms:
        out["max_t"], out["min_t"] = hi, lo
        out["p"] = np.stack([fwe_p(out["t"][j], hi[:, j], lo[:, j] if two_sided else None, out["fit"]) for j in range(len(c))])
    if sink is not None:
        try:
            _read_clusters(sink, out)
        finally:
            sink.close()
    if enhance is not None:
        try:
            _read_tfce(enhance, out)
        finally:
            enhance.close()
    return out


def _glm_slabs(out, grid, X, c, planes, add, region, fit, device, smooth, moves, sink, enhance):
    """group_glm()'s slab loop: per slab a GroupGLM, add(acc, k) for every design row, the fit with `fit` = (min_count, sigma_floor,
    fill) into `out`, and with `moves` = (perm, sign, columns) one permute call for the extrema, which fills `sink` if there is
    one, and one more that fills `enhance`.  Returns (max_t, min_t) over the grid, (None, None) without permutations."""
    min_count, sigma_floor, fill = fit
    depth = int(grid[0][2])
    hi = lo = None
    for first in range(0, depth, planes):
        m = min(planes, depth - first)
        acc = GroupGLM(grid, X, (first, m), device, smooth)
        try:
            for k in range(len(X)):
                add(acc, k)
            r = None if region is None else region[first:first + m]
            b, s, t, k = acc.finish(c, min_count, sigma_floor, r, fill)
            marked = acc.finish(c, min_count, sigma_floor, r, -1.0)[1]      # a residual stdev is never -1: the unfit voxels
            sl = slice(first, first + m)
            out["beta"][:, sl], out["sigma"][sl], out["t"][:, sl], out["count"][sl], out["fit"][sl] = b, s, t, k, marked != -1
            if moves is not None:
                perm, sign, columns = moves
                h, l = acc._permute(sink, 0, c, perm, sign, columns, min_count, sigma_floor, r)
                if enhance is not None:
                    acc._permute(enhance, 0, c, perm, sign, columns, min_count, sigma_floor, r)
                if hi is None:
                    hi, lo = h, l
                else:
                    hi, lo = np.where(_float_keys(h) > _float_keys(hi), h, hi), np.where(_float_keys(l) < _float_keys(lo), l, lo)
        finally:
            acc.close()
    return hi, lo


def _read_clusters(sink, out):
    """group_glm()'s max_extent, clusters, cluster_extent and cluster_p into `out`, from the ClusterSink every slab has filled."""
    n_c, shape = sink.n_contrasts, sink.shape
    out["max_extent"] = sink.finish().max(axis=2)
    out["clusters"], out["cluster_extent"], out["cluster_p"] = np.zeros((n_c,) + shape, np.int32), [], np.ones((n_c,) + shape, np.float32)
    for j in range(n_c):
        k = 0
        for side in range(sink.sides):
            labels, n = sink.labels(0, j, side)
            out["clusters"][j][labels != 0] = labels[labels != 0].astype(np.int32) + k
            k += n
        extent = np.bincount(out["clusters"][j].reshape(-1), minlength=k + 1)[1:].astype(np.uint32)
        out["cluster_extent"].append(extent)
        p = np.concatenate([np.ones(1, np.float32), cluster_p(extent, out["max_extent"][:, j])])
        out["cluster_p"][j] = p[out["clusters"][j]]


def _read_tfce(enhance, out):
    """group_glm()'s max_tfce, tfce and tfce_p into `out`, from the TfceSink every slab has filled."""
    n_c = enhance.n_contrasts
    out["max_tfce"] = enhance.finish().max(axis=2)
    out["tfce"] = np.stack([enhance.map(0, j, 0) for j in range(n_c)])
    if enhance.sides == 2:
        out["tfce"] -= np.stack([enhance.map(0, j, 1) for j in range(n_c)])      # a voxel has at most one side
    out["tfce_p"] = np.stack([tfce_p(out["tfce"][j], out["max_tfce"][:, j]) for j in range(n_c)])


FUSED_DTYPES = ("uint8", "uint16", "int16", "int32", "uint32")


class ModeImages(_Accumulator):
    """frog_modes (include/frog_chain.h): `components` (3: displacements, 1: a scalar) float32 per added image and voxel of a
    window of `grid`, then the Gram matrix of the centred images over the voxels every image covers, and the mean and the modes
    that a set of weights gives.  `window` = (first z-plane, planes), default the whole grid."""

    _NAME = "modes"

    def __init__(self, grid, n_images, components=3, window=None, device=0):
        first, planes = (0, int(grid[0][2])) if window is None else (int(window[0]), int(window[1]))
        super().__init__(grid, first, planes, int(n_images), int(components), int(device))
        self.n_images, self.components = int(n_images), int(components)
        self.window = (first, planes)
        self.shape = (planes,) + self.dims[1::-1]
        self.value_shape = self.shape + ((3,) if self.components == 3 else ())

    def _geometry(self, support):
        if support is None:
            return None
        dims, origin, spacing = support
        return C.byref(_abi.volume_view(None, tuple(float(v) for v in origin), tuple(float(v) for v in spacing), tuple(int(d) for d in dims)))

    def add(self, volume, chain=None, mask=None, interpolation=1, background=0.0):
        """One component: what GroupGLM.add stores."""
        _, src, mv, _, _ = self._views(volume, mask)
        _abi.check(self._lib.frog_modes_add(self._h, chain._h if chain is not None else None, src, mv, int(interpolation),
                                            float(background)), "frog_modes_add")

    def add_jacobian(self, chain, support=None, mask=None, log=True):
        """One component: what GroupGLM.add_jacobian stores."""
        mv = self._views(mask)[1] if mask is not None else None
        _abi.check(self._lib.frog_modes_add_jacobian(self._h, chain._h if chain is not None else None, self._geometry(support), mv,
                                                     int(bool(log))), "frog_modes_add_jacobian")

    def add_displacement(self, chain, support=None, mask=None):
        """Three components: the displacement of `chain` at every window voxel, what Chain.sample gives there as float32;
        `support` and `mask` as in add_jacobian."""
        mv = self._views(mask)[1] if mask is not None else None
        _abi.check(self._lib.frog_modes_add_displacement(self._h, chain._h if chain is not None else None, self._geometry(support), mv),
                   "frog_modes_add_displacement")

    def plane(self, image_index):
        """What add number image_index stored over the window: float32 shape (+ (3,)), NaN (0x7FC00000) where it takes no part."""
        out = np.empty(self.value_shape, np.float32)
        _abi.check(self._lib.frog_modes_plane(self._h, int(image_index), out.ctypes.data_as(_abi.c_float_p)), "frog_modes_plane")
        return out

    def _region(self, region):
        r = None if region is None else np.ascontiguousarray(np.asarray(region) != 0, np.uint8)
        if r is not None and r.shape != self.shape:
            raise ValueError("region: one value per window voxel")
        return r, None if r is None else r.ctypes.data_as(C.POINTER(C.c_uint8))

    def gram(self, region=None, gram=None, n_support=0):
        """(gram, n_support): the packed lower triangle, float64 (n (n + 1) / 2,), of the centred images' inner products over
        the window's support, added onto `gram` (default zeros), and the support's voxels added to n_support.  Windows that
        partition the grid give the whole grid's bits when they are taken in ascending order with gram passed on."""
        n = self.n_images
        g = np.zeros(n * (n + 1) // 2, np.float64) if gram is None else np.array(gram, np.float64).ravel()
        if len(g) != n * (n + 1) // 2:
            raise ValueError("gram: the packed lower triangle of n_images x n_images expected")
        _r, rp = self._region(region)
        count = C.c_uint64(int(n_support))
        _abi.check(self._lib.frog_modes_gram(self._h, rp, g.ctypes.data_as(_abi.c_double_p), C.byref(count)), "frog_modes_gram")
        return g, count.value

    def project(self, weights, region=None, fill=0.0):
        """(mean, modes): float32 of value shape and (n_modes,) + value shape; mode k is the sum over the images of weights[k, i]
        times the centred image i.  `fill` outside the support."""
        w = np.ascontiguousarray(weights, np.float64).reshape(-1, self.n_images)
        _r, rp = self._region(region)
        mean = np.empty(self.value_shape, np.float32)
        modes = np.empty((len(w),) + self.value_shape, np.float32)
        _abi.check(self._lib.frog_modes_project(self._h, rp, len(w), w.ctypes.data_as(_abi.c_double_p), float(fill),
                                                mean.ctypes.data_as(_abi.c_float_p), modes.ctypes.data_as(_abi.c_float_p)), "frog_modes_project")
        return mean, modes


def modes_planes(grid, n_images, components=3, device=0):
    """The most z-planes of `grid` a ModeImages window for n_images may hold on the device now (frog_modes_planes)."""
    dims, origin, spacing = grid
    g = _abi.volume_view(None, origin, spacing, tuple(int(d) for d in dims))
    planes = C.c_uint32()
    _abi.check(_abi.hip_lib().frog_modes_planes(C.byref(g), int(n_images), int(components), int(device), C.byref(planes)), "frog_modes_planes")
    return planes.value


def modes_eigen(gram, divisor=1.0):
    """(values float64 (n,), vectors float64 (n, n)) of the symmetric matrix whose packed lower triangle is `gram`, divided by
    `divisor` (frog_modes_eigen: cyclic Jacobi): values descend, row k of vectors is the unit eigenvector of values[k] with its
    entry of largest magnitude positive.  Host code: no device is needed."""
    g = np.ascontiguousarray(gram, np.float64).ravel()
    n = int(round((np.sqrt(8 * len(g) + 1) - 1) / 2))
    if n * (n + 1) // 2 != len(g):
        raise ValueError("gram: a packed lower triangle expected")
    values, vectors = np.empty(n, np.float64), np.empty((n, n), np.float64)
    _abi.check(_abi.hip_lib().frog_modes_eigen(n, g.ctypes.data_as(_abi.c_double_p), float(divisor), values.ctypes.data_as(_abi.c_double_p),
                                               vectors.ctypes.data_as(_abi.c_double_p)), "frog_modes_eigen")
    return values, vectors


def drop_linear(links):
    """A chain's links without the linear ones: its deformable part (bin/GroupModes -nl 1)."""
    from .chain import LINEAR
    return [l for l in links if l.kind != LINEAR]


def group_modes(chains=None, grid=None, value="displacement", volumes=None, masks=None, supports=None, region=None, n_modes=None,
                fill=0.0, mode_sd=0.0, interpolation=1, max_planes=None, device=0):
    """The principal modes of a registered group (bin/GroupModes): the statistical deformation model of Rueckert, Frangi and
    Schnabel (2003).  value "displacement" (3 components): image i is the displacement of chains[i] on `grid` in mm;
    "logjacobian", "jacobian" and "images" as in group_glm().  A voxel belongs to the SUPPORT where `region` (optional) is
    non-zero and every image takes part.  n_modes: the modes kept, default min(n - 1, 8).
    The device holds slabs of modes_planes() z-planes (at most max_planes).  With one slab the images are added once; with more
    they are added twice, once for the Gram matrix (the slabs in ascending order, which the stated sums need) and, after the
    eigen-solve on the host, once more for the projection.
    Returns a dict: mean float32 value-shaped, modes float32 (n_modes,) + value shape in units per standard deviation (`fill`
    outside the support in both), support uint8, n_support, gram (packed), eigenvalues and vectors (all n, of gram / (n - 1)),
    rms, share, cumulative (n_modes,), scores float64 (n, n_modes) in standard deviations, distance (n,) = the norm of an image's
    scores, distance_robust_z = robust_z(distance).  With mode_sd = s > 0 (displacement only) also mean_field and plus, minus
    (n_modes,) + value shape, float32: mean and mean +- s * mode_k as displacement fields, 0 outside the support."""
    kinds = ("displacement", "logjacobian", "jacobian", "images")
    if value not in kinds:
        raise ValueError("value: " + ", ".join(kinds))
    images = value == "images"
    if images:
        vols, grid = _group(volumes, chains, masks, grid)
        n = len(vols)
    elif chains is None or grid is None:
        raise ValueError("a grid and one chain per image expected")
    else:
        n = len(chains)
    if n < 2:
        raise ValueError("at least two images expected")
    components = 3 if value == "displacement" else 1
    if mode_sd and components != 3:
        raise ValueError("mode_sd: displacement fields only")
    keep = min(n - 1, 8) if n_modes is None else int(n_modes)
    if not 1 <= keep <= n:
        raise ValueError("n_modes: 1 to the number of images")
    dims = tuple(int(d) for d in grid[0])
    depth, shape = dims[2], dims[::-1]
    value_shape = shape + ((3,) if components == 3 else ())
    reg = None if region is None else np.asarray(region) != 0
    planes = modes_planes(grid, n, components, device)
    if max_planes is not None:
        planes = max(1, min(planes, int(max_planes)))

    def filled(first, m):
        acc = ModeImages(grid, n, components, (first, m), device)
        try:
            for k in range(n):
                mask = None if masks is None else masks[k]
                support = None if supports is None else supports[k]
                if images:
                    acc.add(vols[k], None if chains is None else chains[k], mask, interpolation)
                elif components == 3:
                    acc.add_displacement(chains[k], support, mask)
                else:
                    acc.add_jacobian(chains[k], support, mask, value == "logjacobian")
        except Exception:
            acc.close()
            raise
        return acc

    slabs = [(first, min(planes, depth - first)) for first in range(0, depth, planes)]
    gram, n_support, kept = None, 0, None
    for first, m in slabs:
        acc = filled(first, m)
        try:
            gram, n_support = acc.gram(None if reg is None else reg[first:first + m], gram, n_support)
        except Exception:
            acc.close()
            raise
        if len(slabs) == 1:
            kept = acc
        else:
            acc.close()
    try:
        if not n_support:
            raise ValueError("the support is empty: no voxel is covered by every image")
        values, vectors = modes_eigen(gram, n - 1)
        root = float(np.sqrt(np.float64(n - 1)))
        weights = vectors[:keep] / root
        out = dict(mean=np.empty(value_shape, np.float32), modes=np.empty((keep,) + value_shape, np.float32), support=np.empty(shape, np.uint8))
        for first, m in slabs:
            acc = kept if kept is not None else filled(first, m)
            try:
                # a mean is never NaN inside the support: NaN as the fill marks the voxels outside it
                mean, modes = acc.project(weights, None if reg is None else reg[first:first + m], np.nan)
            finally:
                if kept is None:
                    acc.close()
            inside = ~np.isnan(mean if components == 1 else mean[..., 0])
            mean[~inside], modes[:, ~inside] = fill, fill
            sl = slice(first, first + m)
            out["mean"][sl], out["modes"][:, sl], out["support"][sl] = mean, modes, inside
    finally:
        if kept is not None:
            kept.close()
    trace = 0.0
    for v in values:
        trace = trace + float(v)
    share = np.array([float(v) / trace if trace > 0 else 0.0 for v in values[:keep]], np.float64)
    scores = root * vectors[:keep].T
    distance = np.empty(n, np.float64)
    for i in range(n):
        s = 0.0
        for k in range(keep):
            s = s + float(scores[i, k]) * float(scores[i, k])
        distance[i] = np.sqrt(s)
    cumulative, c = np.empty(keep, np.float64), 0.0
    for k in range(keep):
        c = c + float(share[k])
        cumulative[k] = c
    per_value = float(n_support) * components
    out.update(n_support=n_support, gram=gram, eigenvalues=values, vectors=vectors, share=share, cumulative=cumulative,
               rms=np.array([np.sqrt(max(float(v), 0.0) / per_value) for v in values[:keep]], np.float64),
               scores=scores, distance=distance, distance_robust_z=robust_z(distance))
    if mode_sd:
        inside = out["support"] != 0
        step = np.float32(mode_sd) * out["modes"]
        out["mean_field"] = np.where(inside[..., None], out["mean"], np.float32(0))
        out["plus"] = np.where(inside[None, ..., None], out["mean"][None] + step, np.float32(0))
        out["minus"] = np.where(inside[None, ..., None], out["mean"][None] - step, np.float32(0))
    return out


def write_group_modes(result, grid, out_dir, mode_sd=0.0):
    """The files bin/GroupModes writes, from group_modes()'s dict: mean.nii.gz, mode_<k>.nii.gz, support.nii.gz, modes.csv and
    scores.csv, and with mode_sd mean_field.nii.gz, mean.json and per mode mode_<k>_plus / _minus .nii.gz and .json."""
    import os
    dims, origin, spacing = grid
    d, o, s = (C.c_uint32 * 3)(*[int(v) for v in dims]), (C.c_double * 3)(*[float(v) for v in origin]), (C.c_double * 3)(*[float(v) for v in spacing])

    def field(name, a):
        a = np.ascontiguousarray(a, np.float32)
        path = os.path.join(str(out_dir), name)
        rc = _abi.host_lib().frog_nifti_write(path.encode(), d, s, o, 3 if a.ndim == 4 else 1, a.ctypes.data_as(_abi.c_float_p))
        if rc != 0:
            raise IOError(f"cannot write {path}")

    def transform(name, file):
        with open(os.path.join(str(out_dir), name), "w") as f:
            f.write('{"transforms": [{"type": "frogDisplacementField", "file": "%s"}]}\n' % file)

    os.makedirs(str(out_dir), exist_ok=True)
    keep = len(result["modes"])
    field("mean.nii.gz", result["mean"])
    for k in range(keep):
        field(f"mode_{k}.nii.gz", result["modes"][k])
    write_volume(os.path.join(str(out_dir), "support.nii.gz"), result["support"], origin, spacing)
    with open(os.path.join(str(out_dir), "modes.csv"), "w") as f:
        f.write("mode,eigenvalue,rms,share,cumulative\n")
        for k in range(keep):
            f.write("%d,%.17g,%.17g,%.17g,%.17g\n" % (k, result["eigenvalues"][k], result["rms"][k], result["share"][k], result["cumulative"][k]))
    with open(os.path.join(str(out_dir), "scores.csv"), "w") as f:
        f.write("image," + "".join(f"score_{k}," for k in range(keep)) + "distance,distance_robust_z\n")
        for i in range(len(result["scores"])):
            f.write("%d," % i + "".join("%.17g," % v for v in result["scores"][i]) + "%.17g,%.17g\n" % (result["distance"][i], result["distance_robust_z"][i]))
    if mode_sd:
        field("mean_field.nii.gz", result["mean_field"])
        transform("mean.json", "mean_field.nii.gz")
        for k in range(keep):
            for side in ("plus", "minus"):
                field(f"mode_{k}_{side}.nii.gz", result[side][k])
                transform(f"mode_{k}_{side}.json", f"mode_{k}_{side}.nii.gz")


def fused_dtype(values):
    """The type bin/FuseLabels gives labels.nii.gz: the first of uint8, uint16, int16, int32, uint32 that holds every label
    value; None if none does."""
    lo, hi = (int(min(values)), int(max(values))) if len(values) else (0, 0)
    for name in FUSED_DTYPES:
        info = np.iinfo(name)
        if info.min <= lo and hi <= info.max:
            return np.dtype(name)
    return None


class _LabelAccumulator(_Accumulator):
    """What Labels, Staple, WeightedLabels and JointLabels share: n_images adds, finish() and the outputs over the sorted
    table of label values, each the library's frog_<_NAME>_<call>."""

    def __init__(self, grid, n_images, *create_args):
        self.n_images = int(n_images)
        self._n_labels = None
        super().__init__(grid, self.n_images, *create_args)

    def _call(self, name):
        return getattr(self._lib, f"frog_{self._NAME}_{name}")

    def finish(self):
        """The number of distinct labels, after exactly n_images adds."""
        n = C.c_uint32()
        _abi.check(self._call("finish")(self._h, C.byref(n)), f"frog_{self._NAME}_finish")
        self._n_labels = int(n.value)
        return self._n_labels

    def values(self):
        """The distinct label values, int64 ascending."""
        values = np.empty(self._n_labels or 0, np.int64)
        _abi.check(self._call("values")(self._h, values.ctypes.data_as(C.POINTER(C.c_int64))), f"frog_{self._NAME}_values")
        return values

    def fused(self, dtype=None, fill_label=None):
        """(labels, second): the fused map as `dtype`, default the first of uint8, uint16, int16, int32, uint32 that holds
        every label (and `fill_label`, which only the accumulators that have one pass on), and its float32 companion."""
        fill = () if fill_label is None else (int(fill_label),)
        if dtype is None:
            dtype = fused_dtype(list(self.values()) + list(fill))
            if dtype is None:
                raise ValueError("no integer type of at most 32 bits holds every label value")
        labels = np.empty(self.dims[::-1], np.dtype(dtype))
        second = np.empty(self.dims[::-1], np.float32)
        lv = _abi.volume_view(labels, tuple(self._grid.origin), tuple(self._grid.spacing))
        _abi.check(self._call("fused")(self._h, *fill, C.byref(lv), second.ctypes.data_as(_abi.c_float_p)), f"frog_{self._NAME}_fused")
        return labels, second

    def probability(self, value):
        """float32 per voxel, for label `value`: of Labels the share of the images that carry it; of Staple the probability
        that the truth is it; of WeightedLabels and JointLabels the share of the voxel's total score that it holds, 0 where
        no weight arrived."""
        p = np.empty(self.dims[::-1], np.float32)
        _abi.check(self._call("probability")(self._h, int(value), p.ctypes.data_as(_abi.c_float_p)), f"frog_{self._NAME}_probability")
        return p


class Labels(_LabelAccumulator):
    """frog_labels (include/frog_chain.h): n_images label maps added one by one on `grid` = (dims(x, y, z), origin, spacing),
    then the majority vote, its agreement, per-label probabilities and the table of vote sums."""

    _NAME = "labels"

    def __init__(self, grid, n_images, max_labels=0, device=0):
        super().__init__(grid, n_images, int(max_labels), int(device))

    def add(self, volume, chain=None, background=0.0, resliced=False):
        """Adds the integer label map `volume` ((voxels, origin, spacing) or an array already on the grid when chain is
        None); with a chain (frog_amd.chain.Chain, grid space -> volume space) its labels are what Chain.reslice gives with
        nearest-neighbour interpolation.  resliced=True returns that volume (source dtype, shape dims[::-1])."""
        _, src, _, ov, out = self._views(volume, None, resliced)
        _abi.check(self._lib.frog_labels_add(self._h, chain._h if chain is not None else None, src, float(background), ov),
                   "frog_labels_add")
        return out

    def values(self):
        """The distinct label values, int64 ascending: the first column of table()."""
        return self.table()[0]

    def table(self):
        """(values int64 ascending, voxels uint64, pairs uint64): per label the votes summed over the voxels and the image
        pairs that agree on it, summed over the voxels."""
        n = self._n_labels or 0
        values, voxels, pairs = np.empty(n, np.int64), np.empty(n, np.uint64), np.empty(n, np.uint64)
        _abi.check(self._lib.frog_labels_table(self._h, values.ctypes.data_as(C.POINTER(C.c_int64)),
                                               voxels.ctypes.data_as(C.POINTER(C.c_uint64)), pairs.ctypes.data_as(C.POINTER(C.c_uint64))),
                   "frog_labels_table")
        return values, voxels, pairs

    def fused(self, dtype=None):
        """(labels, agreement): the majority label per voxel (ties: the smallest value) as `dtype`, default the first of
        uint8, uint16, int16, int32, uint32 that holds every label; float32 share of the images that voted for it."""
        return super().fused(dtype)


def group_dice(voxels, pairs, n_images):
    """The pooled pairwise Dice overlap per label, 2 pairs / ((n_images - 1) voxels) in float64 (include/frog_chain.h); NaN
    for a single image."""
    voxels, pairs = np.asarray(voxels, np.float64), np.asarray(pairs, np.float64)
    if n_images < 2:
        return np.full(voxels.shape, np.nan)
    return 2.0 * pairs / ((n_images - 1.0) * voxels)


def fuse_labels(volumes, chains=None, grid=None, background=0.0, max_labels=0, device=0):
    """Majority-vote fusion of a group's label maps on the device (bin/FuseLabels).  `volumes`, `chains` and `grid` as in
    average(); every volume has an integer type.  Returns (labels, agreement, values, dice): the fused map, the float32
    share of the images that agree with it, the distinct label values in ascending order and per label the pooled pairwise
    Dice overlap across the group (float64)."""
    vols, grid = _group(volumes, chains, None, grid)
    acc = Labels(grid, len(vols), max_labels, device)
    try:
        for k, v in enumerate(vols):
            acc.add(v, None if chains is None else chains[k], background)
        acc.finish()
        values, voxels, pairs = acc.table()
        labels, agreement = acc.fused()
        return labels, agreement, values, group_dice(voxels, pairs, len(vols))
    finally:
        acc.close()


class Staple(_LabelAccumulator):
    """frog_staple (include/frog_chain.h): n_images label maps added one by one on `grid` = (dims(x, y, z), origin, spacing),
    then multi-label STAPLE: an EM consensus that weights every image's vote by its estimated confusion matrix, and those
    matrices.  At most 256 distinct labels and 4096 images."""

    _NAME = "staple"

    def __init__(self, grid, n_images, max_labels=0, device=0):
        super().__init__(grid, n_images, int(max_labels), int(device))

    def add(self, volume, chain=None, background=0.0, resliced=False):
        """As Labels.add: the integer label map `volume`, through `chain` with nearest-neighbour interpolation."""
        _, src, _, ov, out = self._views(volume, None, resliced)
        _abi.check(self._lib.frog_staple_add(self._h, chain._h if chain is not None else None, src, float(background), ov),
                   "frog_staple_add")
        return out

    def solve(self, p0=0.99, tol=1e-6, max_iter=50, restrict=False):
        """Runs the EM from theta = p0 on the diagonal until the largest change of a theta entry is below `tol` or max_iter
        M-steps ran; restrict=True leaves the voxels at which all images agree out of it.  May be called again.  Returns
        (iterations, change, active_voxels)."""
        p0, tol, max_iter = float(p0), float(tol), int(max_iter)
        if not 0 <= max_iter < 2 ** 32:
            raise ValueError("max_iter from 0 to 2^32 - 1")
        it, change, active = C.c_uint32(), C.c_double(), C.c_uint64()
        _abi.check(self._lib.frog_staple_solve(self._h, p0, tol, max_iter, int(bool(restrict)), C.byref(it), C.byref(change),
                                               C.byref(active)), "frog_staple_solve")
        return int(it.value), float(change.value), int(active.value)

    def fused(self, dtype=None):
        """(labels, confidence): per voxel the label with the largest probability (ties: the smallest value) as `dtype`,
        default the first of uint8, uint16, int16, int32, uint32 that holds every label; its float32 probability."""
        return super().fused(dtype)

    def performance(self):
        """(theta, sums, totals, prior): theta[i, l', l] = P(image i shows values[l'] | the truth is values[l]), float64; the
        uint64 sums[i, l', l] and totals[l] of the last M-step, whose quotient theta is; the float64 prior[l]."""
        n, L = self.n_images, self._n_labels or 0
        theta, sums = np.empty((n, L, L), np.float64), np.empty((n, L, L), np.uint64)
        totals, prior = np.empty(L, np.uint64), np.empty(L, np.float64)
        _abi.check(self._lib.frog_staple_performance(self._h, theta.ctypes.data_as(_abi.c_double_p), sums.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                     totals.ctypes.data_as(C.POINTER(C.c_uint64)), prior.ctypes.data_as(_abi.c_double_p)),
                   "frog_staple_performance")
        return theta, sums, totals, prior


def staple_accuracy(sums, totals):
    """Per image sum_l S[i][l][l] / sum_l T[l]: u64 sums, one float64 division (performance.csv's accuracy)."""
    sums, totals = np.asarray(sums, np.uint64), np.asarray(totals, np.uint64)
    diagonal = np.trace(sums, axis1=1, axis2=2, dtype=np.uint64)
    return diagonal.astype(np.float64) / np.float64(totals.sum(dtype=np.uint64))


def staple_labels(volumes, chains=None, grid=None, background=0.0, p0=0.99, tol=1e-6, max_iter=50, restrict=False, max_labels=0,
                  device=0):
    """STAPLE fusion of a group's label maps on the device (bin/FuseLabels -s 1).  `volumes`, `chains` and `grid` as in
    average(); every volume has an integer type.  Returns a dict: labels, confidence, values, theta, sums, totals, prior
    (Staple.performance), accuracy (staple_accuracy), iterations, change, active_voxels."""
    vols, grid = _group(volumes, chains, None, grid)
    acc = Staple(grid, len(vols), max_labels, device)
    try:
        for k, v in enumerate(vols):
            acc.add(v, None if chains is None else chains[k], background)
        acc.finish()
        iterations, change, active = acc.solve(p0, tol, max_iter, restrict)
        labels, confidence = acc.fused()
        theta, sums, totals, prior = acc.performance()
        return {"labels": labels, "confidence": confidence, "values": acc.values(), "theta": theta, "sums": sums, "totals": totals,
                "prior": prior, "accuracy": staple_accuracy(sums, totals), "iterations": iterations, "change": change,
                "active_voxels": active}
    finally:
        acc.close()


class WeightedLabels(_LabelAccumulator):
    """frog_wlabels (include/frog_chain.h): locally weighted label fusion.  The target image first, then n_images atlases
    (image + label map through one chain) on `grid` = (dims(x, y, z), origin, spacing); every atlas votes for its label with
    the local normalised cross-correlation between its image and the target over a (2 radius + 1)^3 patch, raised to
    `power` and at least `floor`.  Then the fused map, its confidence and per-label probabilities."""

    _NAME = "wlabels"

    def __init__(self, grid, n_images, max_labels=0, radius=2, power=2, floor=2.0 ** -10, device=0):
        super().__init__(grid, n_images, int(max_labels), int(radius), int(power), float(floor), int(device))

    def target(self, volume, chain=None, interpolation=1, background=0.0, resliced=False):
        """The image to segment ((voxels, origin, spacing) or an array already on the grid when chain is None), once, before
        the first add; with a chain (frog_amd.chain.Chain, grid space -> volume space) it is resliced as Chain.reslice does.
        resliced=True returns that volume (source dtype, shape dims[::-1])."""
        _, src, _, ov, out = self._views(volume, None, resliced)
        _abi.check(self._call("target")(self._h, chain._h if chain is not None else None, src, int(interpolation), float(background), ov),
                   f"frog_{self._NAME}_target")
        return out

    def add(self, image, labels, chain=None, interpolation=1, image_background=0.0, label_background=0.0, resliced=False):
        """One atlas: `image` and the integer label map `labels` (each (voxels, origin, spacing) with its own geometry, or an
        array already on the grid when chain is None) through one chain.  resliced=True returns (image, labels) as
        Chain.reslice gives them (the labels with nearest-neighbour interpolation)."""
        _, src, _, ov, out = self._views(image, None, resliced)
        _, lsrc, _, lv, lout = self._views(labels, None, resliced)
        _abi.check(self._call("add")(self._h, chain._h if chain is not None else None, src, lsrc, int(interpolation),
                                     float(image_background), float(label_background), ov, lv), f"frog_{self._NAME}_add")
        return (out, lout) if resliced else None

    def fused(self, dtype=None, fill_label=0):
        """(labels, confidence): per voxel the label with the largest score (ties: the smallest value) as `dtype`, default
        the first of uint8, uint16, int16, int32, uint32 that holds every label and `fill_label`; float32 share of the
        voxel's total score that went to it.  Where no weight arrived: `fill_label`, confidence 0."""
        return super().fused(dtype, fill_label)


class JointLabels(WeightedLabels):
    """frog_jlabels (include/frog_chain.h): joint label fusion (Wang et al., PAMI 2013).  The calls of WeightedLabels; an add
    only collects, and finish() solves, per voxel, the n x n system of the atlases' pairwise patch differences from the target
    (raised elementwise to `beta`, `alpha` on the diagonal) for the weights of the vote, which sum to 1 and may be negative.
    At most 32 atlases, radius 1..3.  keep_weights=True keeps every atlas' weight plane for weight()."""

    _NAME = "jlabels"

    def __init__(self, grid, n_images, max_labels=0, radius=2, beta=2, alpha=0.1, keep_weights=False, device=0):
        _LabelAccumulator.__init__(self, grid, n_images, int(max_labels), int(radius), int(beta), float(alpha), int(bool(keep_weights)),
                                   int(device))

    def weight(self, image_index):
        """float32 weight of atlas `image_index` (in call order) per voxel, 0 where it is not active; after finish()."""
        w = np.empty(self.dims[::-1], np.float32)
        _abi.check(self._lib.frog_jlabels_weight(self._h, int(image_index), w.ctypes.data_as(_abi.c_float_p)), "frog_jlabels_weight")
        return w


def atlas_segment(target, images, label_maps, chains=None, target_chain=None, grid=None, radius=2, power=2, floor=2.0 ** -10,
                  interpolation=1, image_backgrounds=None, label_background=0.0, fill_label=0, max_labels=0, device=0):
    """Multi-atlas segmentation of `target` by locally weighted voting (bin/AtlasSegment).  `images`, `chains` and `grid` as
    in average(); `label_maps`: one integer volume per image, with its own geometry; `target_chain`: None (the target is on
    the grid) or the Chain from grid space to the target's; `image_backgrounds`: None (each volume's minimum, the target's
    included), a number or one per image.  Returns (labels, confidence, values): the fused map in the grid's space, the
    float32 share of each voxel's score that its label holds, and the distinct label values in ascending order."""
    acc_of = lambda grid, n: WeightedLabels(grid, n, max_labels, radius, power, floor, device)
    return _segment(acc_of, target, images, label_maps, chains, target_chain, grid, interpolation, image_backgrounds, label_background,
                    fill_label)[:3]


def joint_atlas_segment(target, images, label_maps, chains=None, target_chain=None, grid=None, radius=2, beta=2, alpha=0.1,
                        interpolation=1, image_backgrounds=None, label_background=0.0, fill_label=0, max_labels=0, keep_weights=False,
                        device=0):
    """atlas_segment() by joint label fusion (bin/AtlasSegment -j 1; JointLabels): the same arguments with `beta` and `alpha`
    in place of `power` and `floor`, at most 32 atlases, radius 1..3.  Returns (labels, confidence, values), and with
    keep_weights a fourth item: the float32 weight plane of every atlas."""
    acc_of = lambda grid, n: JointLabels(grid, n, max_labels, radius, beta, alpha, keep_weights, device)
    out = _segment(acc_of, target, images, label_maps, chains, target_chain, grid, interpolation, image_backgrounds, label_background,
                   fill_label, keep_weights)
    return out if keep_weights else out[:3]


def _segment(acc_of, target, images, label_maps, chains, target_chain, grid, interpolation, image_backgrounds, label_background, fill_label,
             weights=False):
    """What atlas_segment() and joint_atlas_segment() share: the target, the adds, finish and the fused map."""
    vols, grid = _group(images, chains, None, grid)
    labels = [_as_volume(v) for v in label_maps]
    if len(labels) != len(vols):
        raise ValueError("one label map per image expected")
    tgt = _as_volume(target)
    if image_backgrounds is None:
        image_backgrounds = [float(a.min()) for a, _, _ in vols]
    elif np.ndim(image_backgrounds) == 0:
        image_backgrounds = [float(image_backgrounds)] * len(vols)
    acc = acc_of(grid, len(vols))
    try:
        acc.target(tgt, target_chain, interpolation, float(tgt[0].min()))
        for k, v in enumerate(vols):
            acc.add(v, labels[k], None if chains is None else chains[k], interpolation, image_backgrounds[k], label_background)
        acc.finish()
        fused, confidence = acc.fused(None, fill_label)
        return fused, confidence, acc.values(), [acc.weight(k) for k in range(len(vols))] if weights else None
    finally:
        acc.close()


SURFACE_ROW = np.dtype([("n_a", np.uint64), ("n_b", np.uint64), ("sum_ab", np.uint64), ("sum_ba", np.uint64),
                        ("max_ab", np.uint32), ("max_ba", np.uint32), ("pct_ab", np.uint32), ("pct_ba", np.uint32)])
assert SURFACE_ROW.itemsize == C.sizeof(_abi.FrogSurfaceRow)


def distance_map(volume, value, spacing=(1.0, 1.0, 1.0), mode=0, device=0):
    """The exact Euclidean distance transform of an integer label map on the device (frog_distance_map,
    include/frog_chain.h): per voxel of `volume`[z, y, x] the distance to the set {volume == value} (mode 0) or to that set's
    surface voxels (mode 1) at `spacing`(x, y, z), as uint32 fixed point in units of 2^-16; 0xFFFFFFFF where the set is
    empty."""
    a = np.ascontiguousarray(volume)
    v = _abi.volume_view(a, (0.0, 0.0, 0.0), tuple(float(s) for s in spacing))
    out = np.empty(a.shape, np.uint32)
    _abi.check(_abi.hip_lib().frog_distance_map(C.byref(v), int(value), int(mode), int(device), out.ctypes.data_as(_abi.c_u32_p)),
               "frog_distance_map")
    return out


class SurfaceDistances(_Accumulator):
    """frog_surface (include/frog_chain.h): the surface distances of label maps to `reference`[z, y, x] for the label
    `values` (strictly ascending).  `grid_or_spacing`: the reference's spacing(x, y, z) (origin 0), or its grid (dims(x, y, z),
    origin, spacing).  The distance maps of the reference are computed once, here."""

    _NAME = "surface"

    def __init__(self, reference, values, grid_or_spacing=(1.0, 1.0, 1.0), percentile=95, device=0):
        self._h = None
        ref = np.ascontiguousarray(reference)
        if ref.ndim != 3:
            raise ValueError("a 3-D reference label map expected")
        if np.ndim(grid_or_spacing[0]) == 0:
            origin, spacing = (0.0, 0.0, 0.0), tuple(float(s) for s in grid_or_spacing)
        else:
            dims, origin, spacing = grid_or_spacing
            if tuple(int(d) for d in dims) != ref.shape[::-1]:
                raise ValueError("the reference's shape differs from the grid's dims")
        if not 0 <= int(percentile) < 2 ** 32:
            raise ValueError("a percentile from 1 to 100")
        self._lib = _abi.hip_lib()
        self.dims = ref.shape[::-1]
        self.values = np.ascontiguousarray(values, np.int64).ravel()
        self.percentile = int(percentile)
        self._grid = _abi.volume_view(None, origin, spacing, self.dims)
        view = _abi.volume_view(ref, origin, spacing)
        h = C.c_void_p()
        _abi.check(self._lib.frog_surface_create(C.byref(view), self.values.ctypes.data_as(C.POINTER(C.c_int64)), len(self.values),
                                                 self.percentile, int(device), C.byref(h)), "frog_surface_create")
        self._h = h

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def add(self, volume, chain=None, background=0.0):
        """One image's rows, a SURFACE_ROW array with an entry per value.  `volume` as in Labels.add: an integer label map
        ((voxels, origin, spacing), or an array already on the grid when chain is None), through `chain` with
        nearest-neighbour interpolation.  Adds are independent of each other."""
        _, src, _, _, _ = self._views(volume)
        rows = np.zeros(len(self.values), SURFACE_ROW)
        _abi.check(self._lib.frog_surface_add(self._h, chain._h if chain is not None else None, src, float(background),
                                              rows.ctypes.data_as(C.POINTER(_abi.FrogSurfaceRow))), "frog_surface_add")
        return rows


def surface_metrics(rows):
    """(hausdorff, hausdorff_p, assd) of SURFACE_ROW rows, float64 in the spacing's unit, by the three lines of
    include/frog_chain.h: max(max_ab, max_ba) * 2^-16, max(pct_ab, pct_ba) * 2^-16 and
    ((sum_ab + sum_ba) / (n_a + n_b)) * 2^-16; NaN where either surface is empty."""
    rows = np.asarray(rows)
    empty = (rows["n_a"] == 0) | (rows["n_b"] == 0)
    scale = 2.0 ** -16
    hausdorff = np.maximum(rows["max_ab"], rows["max_ba"]).astype(np.float64) * scale
    hausdorff_p = np.maximum(rows["pct_ab"], rows["pct_ba"]).astype(np.float64) * scale
    count = np.where(empty, np.uint64(1), rows["n_a"] + rows["n_b"])
    assd = ((rows["sum_ab"] + rows["sum_ba"]).astype(np.float64) / count.astype(np.float64)) * scale
    for m in (hausdorff, hausdorff_p, assd):
        m[empty] = np.nan
    return hausdorff, hausdorff_p, assd


def _mean_in_order(values):
    """The sum of `values` one by one from +0.0, over their number (surface_images.csv and surface_labels.csv form their
    means this way); NaN for none."""
    total = 0.0
    for v in values:
        total = total + float(v)
    return total / len(values) if len(values) else float("nan")


def surface_distances(volumes, reference, values=None, chains=None, grid=None, background=0.0, percentile=95, device=0):
    """The surface distances of a group's label maps to a consensus (bin/FuseLabels -d 1).  `volumes`, `chains` and `grid` as
    in fuse_labels(); `reference`[z, y, x] is an integer label map on the grid; `values`: the labels to measure, default every
    value of the reference except `background`.  Returns a dict: values; rows (SURFACE_ROW, images x values); hausdorff,
    hausdorff_p, assd (surface_metrics of the rows); per image labels_measured, mean_assd, mean_assd_robust_z (robust_z) and
    max_hausdorff over the labels with both surfaces; per label images_measured, label_mean_assd, label_max_hausdorff and
    label_mean_hausdorff_p over the images.  Means are sums in ascending order from +0.0 over the count."""
    vols, grid = _group(volumes, chains, None, grid)
    ref = np.ascontiguousarray(reference)
    if values is None:
        values = [int(v) for v in np.unique(ref) if float(v) != float(background)]
    with SurfaceDistances(ref, values, grid, percentile, device) as acc:
        rows = np.stack([acc.add(v, None if chains is None else chains[k], background) for k, v in enumerate(vols)])
    hausdorff, hausdorff_p, assd = surface_metrics(rows)
    measured = ~np.isnan(assd)
    nan = float("nan")
    out = {"values": np.ascontiguousarray(values, np.int64), "rows": rows, "hausdorff": hausdorff, "hausdorff_p": hausdorff_p, "assd": assd,
           "labels_measured": measured.sum(1), "images_measured": measured.sum(0),
           "mean_assd": np.array([_mean_in_order(a[m]) for a, m in zip(assd, measured)]),
           "max_hausdorff": np.array([h[m].max() if m.any() else nan for h, m in zip(hausdorff, measured)]),
           "label_mean_assd": np.array([_mean_in_order(a[m]) for a, m in zip(assd.T, measured.T)]),
           "label_max_hausdorff": np.array([h[m].max() if m.any() else nan for h, m in zip(hausdorff.T, measured.T)]),
           "label_mean_hausdorff_p": np.array([_mean_in_order(h[m]) for h, m in zip(hausdorff_p.T, measured.T)])}
    out["mean_assd_robust_z"] = robust_z(out["mean_assd"])
    return out
